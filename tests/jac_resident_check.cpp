// Stand-alone check of the resident dense-Jacobian table (pyneuralempc_amd/csrc/jac_resident.h: plain host code).
// Built and run by tests/test_jac_resident_cpu.py with -fsanitize=address,undefined.  Pointers are never dereferenced:
// they are addresses inside one array.
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
    auto t = std::make_unique<JacResidentTable>();     // (on the heap: a read past the table is the sanitizer's to see)

    // ---- empty table, null pointers, lookup
    CHECK(t->count() == 0);
    CHECK(!t->resident(P(0), 1) && !t->resident(nullptr, 1) && !t->find(nullptr));
    CHECK(!t->add(nullptr, 4) && !t->add(P(0), 0) && !t->add(P(0), -1) && t->count() == 0);
    CHECK(!t->remove(P(0)) && !t->remove(nullptr));
    CHECK(t->add(P(0), 7) && t->count() == 1);
    CHECK(t->find(P(0)) && t->find(P(0))->B == 7 && !t->find(P(1)));

    // ---- B limit: up to the registered B, not beyond
    CHECK(t->resident(P(0), 1) && t->resident(P(0), 4) && t->resident(P(0), 7));
    CHECK(!t->resident(P(0), 8) && !t->resident(P(1), 1));
    // registering again keeps the slot and takes the new B (smaller or larger)
    CHECK(t->add(P(0), 3) && t->count() == 1 && t->resident(P(0), 3) && !t->resident(P(0), 4));
    CHECK(t->add(P(0), 9) && t->count() == 1 && t->resident(P(0), 9));

    // ---- capacity: kJacResidentSlots entries, the next one is refused and changes nothing
    for (int i = 1; i < kJacResidentSlots; ++i) CHECK(t->add(P(i), i + 1));
    CHECK(t->count() == kJacResidentSlots);
    CHECK(!t->add(P(kJacResidentSlots), 5) && t->count() == kJacResidentSlots && !t->resident(P(kJacResidentSlots), 1));
    for (int i = 1; i < kJacResidentSlots; ++i) CHECK(t->resident(P(i), i + 1) && !t->resident(P(i), i + 2));
    CHECK(t->add(P(3), 2) && t->count() == kJacResidentSlots);      // a pointer it holds is still accepted when full

    // ---- removal frees exactly one slot
    CHECK(t->remove(P(3)) && !t->remove(P(3)) && t->count() == kJacResidentSlots - 1 && !t->resident(P(3), 1));
    CHECK(t->add(P(kJacResidentSlots), 5) && t->count() == kJacResidentSlots && t->resident(P(kJacResidentSlots), 5));
    CHECK(!t->add(P(3), 4));
    for (int i = 0; i < kJacResidentSlots; ++i)
        if (i != 3) CHECK(t->resident(P(i), 1));

    // ---- epoch drop: every entry at once; a dropped pointer registers again like a new one
    t->drop_all();
    CHECK(t->count() == 0);
    for (int i = 0; i <= kJacResidentSlots; ++i) CHECK(!t->resident(P(i), 1) && !t->find(P(i)) && !t->remove(P(i)));
    CHECK(t->add(P(2), 6) && t->count() == 1 && t->resident(P(2), 6) && !t->resident(P(2), 7) && !t->resident(P(0), 1));
    t->drop_all();
    t->drop_all();
    CHECK(t->count() == 0 && !t->resident(P(2), 1));
    for (int i = 0; i < kJacResidentSlots; ++i) CHECK(t->add(P(20 + i), 1));      // all slots usable again
    CHECK(!t->add(P(40), 1));

    // ---- epoch wrap-around: no entry of an earlier epoch comes back to life
    t->epoch = ~0u;
    for (auto& e : t->slot) e.epoch = 1;             // what a table that has seen 2^32 - 2 drops could still hold
    t->drop_all();
    CHECK(t->epoch == 1 && t->count() == 0 && !t->resident(P(20), 1));
    CHECK(t->add(P(20), 2) && t->resident(P(20), 2));

    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
