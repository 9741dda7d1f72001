// Windowed checkpointing of a snapshot stack, as pure integer arithmetic: which forward state lives in which slot, which window a read has to
// replay first, and which interval a context takes from the free HBM.  One schedule for the KDYN context (kdyn.hip: class KDyn, with
// kdyn_plan.hpp) and the Poiseuille contexts (pois.hip: class PoisBase, keep_last).
//
// Host-only: no HIP type is named here, so g++ alone compiles it and tests/c/kdyn_plan_test.cpp walks every schedule of both contexts on the
// CPU (tests/test_kdyn_plan.py).  Nothing here allocates or launches.
#pragma once
#include <algorithm>
#include <cstddef>

namespace smo {
namespace ckpt {

// States 0..N of a forward solve.  Every ck-th state is kept in the stack, the others live in (ck - 1) scratch slots that hold ONE window
// (the states w*ck + 1 .. w*ck + ck - 1) at a time.  Dense tail: from index dense_from (a multiple of ck) on EVERY state is kept — the HBM that
// a uniform interval leaves unused (256^3 x 1000 steps on one GPU: interval 2 = 200 GB of 288) buys that many windows less to recompute.
// pingpong (frozen velocity, keep_states = 0): no stack at all, the forward solve alternates between two slots.
// keep_last (Poiseuille; no tail, no ping-pong): state N is always kept, behind the checkpoints in a stack slot of its own when N is no multiple
// of ck.  The mix-norm cost overwrites snapshot N after the forward loop, so no replay may write it: the last window ends at N - 1.
constexpr int kNoDenseTail = 1 << 30;

struct Slot {
    bool scratch;          // in the scratch window (else: in the stack)
    size_t index;          // slot of that array
};

struct Schedule {
    int N = 0, ck = 1, dense_from = kNoDenseTail;
    bool pingpong = false, keep_last = false;

    bool has_tail() const { return dense_from <= N; }
    bool own_last_slot() const { return keep_last && N % ck != 0; }
    bool kept(int n) const { return n >= dense_from || n % ck == 0 || (keep_last && n == N); }          // lives in the stack for good
    Slot slot(int n) const {
        if (pingpong) return {false, (size_t)(n & 1)};
        if (n >= dense_from) return {false, (size_t)(dense_from / ck) + (size_t)(n - dense_from)};
        if (n == N && own_last_slot()) return {false, (size_t)(N / ck) + 1};
        const int r = n % ck;
        return r == 0 ? Slot{false, (size_t)(n / ck)} : Slot{true, (size_t)(r - 1)};
    }
    size_t stack_slots() const {
        if (pingpong) return 2;
        return has_tail() ? (size_t)(dense_from / ck) + (size_t)(N - dense_from) + 1 : (size_t)N / ck + 1 + (own_last_slot() ? 1 : 0);
    }
    size_t scratch_slots() const { return (size_t)(ck - 1); }
    // windows: state idx belongs to window idx / ck; a state that is not kept can be read while its window is the resident one, else the
    // window is replayed by the forward steps first(w) .. last(w) - 1, which write the states up to last(w)
    int window(int idx) const { return idx / ck; }
    bool resident(int idx, int resident_window) const { return kept(idx) || resident_window == window(idx); }
    int first(int w) const { return w * ck; }
    int last(int w) const { return std::min(keep_last ? N - 1 : N, w * ck + ck - 1); }
    // the window a forward solve leaves in the scratch slots: that of the last state that is not kept (-1: none).  keep_last: that state is
    // N - 1, or N - 2 when N - 1 is a checkpoint, and either lies in window (N - 2) / ck — not (N - 1) / ck, which then starts at N - 1 and has
    // no recomputed state at all
    int window_after_forward() const {
        if (keep_last) return (ck > 1 && N >= 2) ? (N - 2) / ck : -1;
        return (ck > 1 && dense_from > 0) ? (std::min(N, dense_from) - 1) / ck : -1;
    }
    // state n has a slot of the Ty cache while `count` states of window `cached` are held there (cached < 0: nothing is)
    bool in_tycache(int n, int cached, int count) const { return cached >= 0 && n >= cached * ck && n < cached * ck + count; }
};

// ---- ckpt = 0: the interval ------------------------------------------------------------------------------------------------------------
// The first interval k in 1..N whose stack fits: bytes(k) <= avail, compared in the type of avail.  0 when none does: KDyn then takes N (one
// window), Poiseuille reports SMO_ERR_NOMEM with smallest_stack().  The slot count falls up to k ~ sqrt(N) and rises again beyond: the first
// that fits, not the smallest stack.
template <class Bytes, class Avail> inline int first_interval(int N, Bytes bytes, Avail avail) {
    for (int k = 1; k <= N; ++k)
        if (!((Avail)bytes(k) > avail)) return k;
    return 0;
}
template <class Bytes> inline size_t smallest_stack(int N, Bytes bytes) {
    size_t least = bytes(1);
    for (int k = 2; k <= N; ++k) least = std::min(least, (size_t)bytes(k));
    return least;
}

}  // namespace ckpt
}  // namespace smo
