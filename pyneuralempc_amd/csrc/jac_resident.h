// Resident dense-Jacobian buffers of a handle (nempc_jac_dense_resident): plain host code, no HIP types.
//
// Which entries of the dense (B, m, n) Jacobian are structural zeros depends on H, nx, nu and the box rows only, never on
// the iterate, and every caller re-evaluates into the same buffer.  A buffer that was zero-filled once and that nobody but
// nempc_eval of this handle writes therefore keeps its zeros: the evaluation may write the structural non-zeros alone.
// This table says which pointers are such buffers.  It is small and fixed: a caller that finds it full simply stays on the
// full-matrix path.  An entry is live while its epoch is the table's; whatever changes m, n or the dense map bumps the
// epoch, which drops every entry at once (the non-zeros of the old shape would otherwise stay behind as stale values).
//
// The constant non-zeros (the -1 of every defect row, the +1 of every box row) are as fixed as the zeros.  A registration
// leaves the buffer all zero; the first evaluation that finds problems without their constants writes them (one small fill in
// front of its launches) and says so here: an entry counts the leading problems that have them, and the writers skip those
// stores like the zeros.  Counted per problem because an evaluation of fewer problems than registered touches only its own.
#pragma once

namespace nempc {

constexpr int kJacResidentSlots = 8;

struct JacResidentTable {
    struct Entry {
        const void* ptr = nullptr;
        int B = 0;                  // problems the zero fill covered
        unsigned epoch = 0;
        int const_B = 0;            // leading problems whose constant entries are in place (<= B)
    };
    Entry slot[kJacResidentSlots];
    unsigned epoch = 1;

    bool live(const Entry& e) const { return e.ptr != nullptr && e.epoch == epoch; }

    // the live entry of `p`, or null
    const Entry* find(const void* p) const {
        if (!p) return nullptr;
        for (const Entry& e : slot)
            if (live(e) && e.ptr == p) return &e;
        return nullptr;
    }

    // may an evaluation of B problems into `p` leave the structural zeros alone?
    bool resident(const void* p, int B) const {
        const Entry* e = find(p);
        return e && B <= e->B;
    }

    // the leading problems of `p` that hold their constants (0: none, or not registered)
    int const_count(const void* p) const {
        const Entry* e = find(p);
        return e ? e->const_B : 0;
    }

    // the constants of problems [0, B) of `p` are in place now; never beyond the registered B, never fewer than before
    void const_filled(const void* p, int B) {
        for (Entry& e : slot)
            if (live(e) && e.ptr == p && B > e.const_B) e.const_B = B < e.B ? B : e.B;
    }

    // registers `p` for B problems, freshly zero-filled: no constants yet (a pointer already in the table keeps its slot
    // and takes the new B).  false: the table is full, nothing changed
    bool add(const void* p, int B) {
        if (!p || B <= 0) return false;
        Entry* free_slot = nullptr;
        for (Entry& e : slot) {
            if (live(e) && e.ptr == p) {
                e.B = B;
                e.const_B = 0;
                return true;
            }
            if (!live(e) && !free_slot) free_slot = &e;
        }
        if (!free_slot) return false;
        free_slot->ptr = p;
        free_slot->B = B;
        free_slot->epoch = epoch;
        free_slot->const_B = 0;
        return true;
    }

    // false: `p` was not registered
    bool remove(const void* p) {
        for (Entry& e : slot)
            if (live(e) && e.ptr == p) {
                e = Entry{};
                return true;
            }
        return false;
    }

    // every entry at once (the shape or the dense map changed)
    void drop_all() {
        if (++epoch == 0) {           // wrapped: no old entry may come back to life
            for (Entry& e : slot) e = Entry{};
            epoch = 1;
        }
    }

    int count() const {
        int c = 0;
        for (const Entry& e : slot) c += live(e) ? 1 : 0;
        return c;
    }
};

}  // namespace nempc
