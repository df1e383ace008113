// Stand-alone check of the constants count of the resident dense-Jacobian table (pyneuralempc_amd/csrc/jac_resident.h: plain
// host code): which leading problems of a registered buffer hold their constant -1 / +1 entries.  Built and run by
// tests/test_jac_resident_consts_cpu.py with -fsanitize=address,undefined.  Pointers are never dereferenced.
#include <cstdio>
#include <memory>

#include "jac_resident.h"

static int failures = 0, checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            ++failures;                                                    \
            std::printf("line %d: %s\n", __LINE__, #cond);                 \
        }                                                                  \
    } while (0)

int main() {
    using nempc::JacResidentTable;
    using nempc::kJacResidentSlots;
    static double arena[64];
    auto P = [&](int i) { return static_cast<const void*>(arena + i); };
    auto t = std::make_unique<JacResidentTable>();

    // ---- nothing registered: no constants anywhere, marking is a no-op
    CHECK(t->const_count(P(0)) == 0 && t->const_count(nullptr) == 0);
    t->const_filled(P(0), 5);
    t->const_filled(nullptr, 5);
    CHECK(t->count() == 0 && t->const_count(P(0)) == 0);

    // ---- a fresh registration has none; the count grows with the evaluated problems, never shrinks, never passes B
    CHECK(t->add(P(0), 33) && t->const_count(P(0)) == 0);
    t->const_filled(P(0), 17);
    CHECK(t->const_count(P(0)) == 17);
    t->const_filled(P(0), 15);
    CHECK(t->const_count(P(0)) == 17);
    t->const_filled(P(0), 0);
    t->const_filled(P(0), -3);
    CHECK(t->const_count(P(0)) == 17);
    t->const_filled(P(0), 33);
    CHECK(t->const_count(P(0)) == 33);
    t->const_filled(P(0), 40);
    CHECK(t->const_count(P(0)) == 33 && t->find(P(0))->B == 33);
    // another pointer is another buffer
    CHECK(t->add(P(1), 8) && t->const_count(P(1)) == 0 && t->const_count(P(0)) == 33);
    t->const_filled(P(1), 100);
    CHECK(t->const_count(P(1)) == 8 && t->const_count(P(0)) == 33);

    // ---- registering again means a fresh zero fill: the constants are gone, whatever the new B
    CHECK(t->add(P(0), 33) && t->const_count(P(0)) == 0);
    t->const_filled(P(0), 33);
    CHECK(t->add(P(0), 4) && t->const_count(P(0)) == 0 && t->resident(P(0), 4) && !t->resident(P(0), 5));
    t->const_filled(P(0), 33);
    CHECK(t->const_count(P(0)) == 4);

    // ---- removal and a new registration in the freed slot
    CHECK(t->remove(P(0)) && t->const_count(P(0)) == 0);
    t->const_filled(P(0), 3);
    CHECK(t->const_count(P(0)) == 0 && !t->find(P(0)));
    CHECK(t->add(P(2), 6) && t->const_count(P(2)) == 0 && t->const_count(P(1)) == 8);

    // ---- epoch drop: the constants go with the zeros; the slots come back without a count
    t->const_filled(P(2), 6);
    t->drop_all();
    CHECK(t->const_count(P(1)) == 0 && t->const_count(P(2)) == 0);
    t->const_filled(P(2), 6);
    CHECK(t->const_count(P(2)) == 0 && t->count() == 0);
    for (int i = 0; i < kJacResidentSlots; ++i) CHECK(t->add(P(10 + i), 9) && t->const_count(P(10 + i)) == 0);
    for (int i = 0; i < kJacResidentSlots; ++i) t->const_filled(P(10 + i), i + 1);
    for (int i = 0; i < kJacResidentSlots; ++i) CHECK(t->const_count(P(10 + i)) == i + 1);
    // a full table refuses a new pointer: nothing to mark
    CHECK(!t->add(P(30), 9));
    t->const_filled(P(30), 9);
    CHECK(t->const_count(P(30)) == 0);

    // ---- epoch wrap-around: an entry of an earlier epoch does not come back with its count
    t->epoch = ~0u;
    for (auto& e : t->slot) e.epoch = 1;
    t->drop_all();
    CHECK(t->epoch == 1 && t->count() == 0 && t->const_count(P(10)) == 0);
    CHECK(t->add(P(10), 9) && t->const_count(P(10)) == 0);

    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
