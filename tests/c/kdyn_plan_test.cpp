// Host check of the checkpoint schedule the KDYN and Poiseuille contexts share (spheremanopt_amd/csrc/ckpt_plan.hpp) and of KDyn's HBM plan
// (kdyn_plan.hpp), run by tests/test_kdyn_plan.py as a program of its own.  Every schedule with N <= 40 steps is walked the way KDyn::ensure
// and PoisBase::ensure walk it: the slot map must be a bijection onto the allocation, the forward solve, both adjoint sweeps and out-of-order
// snapshot reads must find every state in its slot, and no window may be replayed twice in a monotone sweep.  Poiseuille's schedules
// (keep_last) besides: no replay may write state N, which the cost overwrites after the forward loop, and slot map, slot count and windows
// must be those of the formulas pois.hip held before it used the shared schedule, written out below.  The choices made from the free HBM are
// compared with brute-force searches.  One line "ok <group>" per group, "FAIL ..." on any violation.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "kdyn_plan.hpp"

using namespace smo::kdplan;
using smo::ckpt::Schedule; using smo::ckpt::Slot; using smo::ckpt::kNoDenseTail; using smo::ckpt::first_interval; using smo::ckpt::smallest_stack;

static int fails = 0;
#define REQUIRE(cond, ...)                                       \
    do {                                                         \
        if (!(cond)) {                                           \
            if (fails < 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } \
            ++fails;                                             \
        }                                                        \
    } while (0)

static void group(const char* name, int before, long cases) { if (fails == before) std::printf("ok %s (%ld cases)\n", name, cases); }

// N = 1..40, ck = 1..min(N, 8), dense_from = none or every multiple of ck <= N; keep_last (Poiseuille) without a tail
template <class F> static long for_each_schedule(F f) {
    long cases = 0;
    for (int N = 1; N <= 40; ++N)
        for (int ck = 1; ck <= std::min(N, 8); ++ck) {
            f(Schedule{N, ck, kNoDenseTail, false}); ++cases;
            for (int D = 0; D <= N; D += ck) { f(Schedule{N, ck, D, false}); ++cases; }
            f(Schedule{N, ck, kNoDenseTail, false, true}); ++cases;
        }
    return cases;
}
#define SCHED "N=%d ck=%d dense_from=%d%s: "
#define SCHED_ARGS s.N, s.ck, s.dense_from, s.keep_last ? " keep_last" : ""

// ---- slot map ------------------------------------------------------------------------------------------------------------------------------
static void slot_map(const Schedule& s) {
    std::vector<int> seen(s.stack_slots(), 0);
    for (int n = 0; n <= s.N; ++n) {
        const bool kept = n % s.ck == 0 || n >= s.dense_from || (s.keep_last && n == s.N);
        const Slot q = s.slot(n);
        REQUIRE(s.kept(n) == kept, SCHED "kept(%d)", SCHED_ARGS, n);
        if (kept) {
            REQUIRE(!q.scratch && q.index < seen.size(), SCHED "state %d in %s slot %zu of %zu", SCHED_ARGS, n, q.scratch ? "scratch" : "stack", q.index, seen.size());
            if (!q.scratch && q.index < seen.size()) seen[q.index] += 1;
        } else {
            REQUIRE(q.scratch && q.index == (size_t)(n % s.ck - 1) && q.index < s.scratch_slots(), SCHED "state %d in %s slot %zu", SCHED_ARGS, n,
                    q.scratch ? "scratch" : "stack", q.index);
        }
    }
    for (size_t i = 0; i < seen.size(); ++i) REQUIRE(seen[i] == 1, SCHED "stack slot %zu holds %d states", SCHED_ARGS, i, seen[i]);      // no hole, no overrun
    if (s.keep_last) {
        REQUIRE(s.stack_slots() == (size_t)(s.N / s.ck + 1 + (s.N % s.ck != 0)), SCHED "%zu stack slots", SCHED_ARGS, s.stack_slots());
        if (s.N % s.ck != 0) REQUIRE(s.slot(s.N).index == (size_t)(s.N / s.ck + 1), SCHED "state N in stack slot %zu", SCHED_ARGS, s.slot(s.N).index);
        for (int w = 0; w <= s.N / s.ck; ++w) REQUIRE(s.last(w) <= s.N - 1, SCHED "window %d ends at %d", SCHED_ARGS, w, s.last(w));
    }
    const Schedule p{s.N, 1, kNoDenseTail, true};
    REQUIRE(p.stack_slots() == 2 && p.scratch_slots() == 0, "ping-pong N=%d: %zu + %zu slots", s.N, p.stack_slots(), p.scratch_slots());
    for (int n = 0; n <= s.N; ++n) REQUIRE(!p.slot(n).scratch && p.slot(n).index == (size_t)(n & 1) && p.resident(n, -1), "ping-pong state %d", n);
}

// ---- sweeps: which state each physical slot holds ------------------------------------------------------------------------------------------
struct Sim {
    Schedule s;
    std::vector<int> stack, scratch;
    int resident = -1;
    long replayed = 0;
    bool cost_written = false;                                                                 // keep_last: the cost has overwritten snapshot N
    static constexpr int kCost = -7;
    explicit Sim(const Schedule& s_) : s(s_), stack(s_.stack_slots(), -1), scratch(s_.scratch_slots(), -1) {}
    int& holder(int n) { const Slot q = s.slot(n); return q.scratch ? scratch[q.index] : stack[q.index]; }
    void read(int n, const char* who) {
        const int want = cost_written && n == s.N ? kCost : n;
        REQUIRE(holder(n) == want, SCHED "%s reads state %d and finds %d", SCHED_ARGS, who, n, holder(n));
    }
    void step(int n, const char* who) { read(n, who); holder(n + 1) = n + 1; }                 // forward step n: state n -> state n + 1
    void forward() {
        cost_written = false;
        holder(0) = 0;
        for (int n = 0; n < s.N; ++n) step(n, "forward");
        if (s.keep_last) { read(s.N, "cost"); holder(s.N) = kCost; cost_written = true; }      // (the mix-norm cost: snapshot N = (dx psi, psiz, psi))
        resident = s.window_after_forward();
    }
    void ensure(int idx) {                                                                     // KDyn::ensure without the launches
        if (s.resident(idx, resident)) return;
        const int w = s.window(idx);
        resident = w;
        for (int n = s.first(w); n < s.last(w); ++n) {
            if (s.keep_last) REQUIRE(&holder(n + 1) != &holder(s.N), SCHED "replay step %d writes the slot of state N", SCHED_ARGS, n);
            step(n, "replay"); ++replayed;
        }
    }
    void get(int idx, const char* who) { ensure(idx); read(idx, who); }
};
// steps a monotone sweep over lo..N has to replay: every window with a state that is not kept, but the one the forward solve left, once
// (keep_last: state N is kept and a replay stops at N - 1)
static long expected_replays(const Schedule& s, int lo) {
    std::vector<int> windows;
    for (int idx = s.N; idx >= lo; --idx)
        if (idx % s.ck != 0 && idx < s.dense_from && !(s.keep_last && idx == s.N) && (windows.empty() || windows.back() != idx / s.ck)) windows.push_back(idx / s.ck);
    const int top = s.keep_last ? s.N - 1 : s.N;
    long steps = 0;
    for (size_t i = 1; i < windows.size(); ++i) steps += std::min(top, windows[i] * s.ck + s.ck - 1) - windows[i] * s.ck;      // (windows[0]: resident)
    return steps;
}
static void sweeps(const Schedule& s) {
    for (int cont = 0; cont < 2; ++cont) {
        Sim m(s);
        m.forward();
        for (int n = 0; n <= s.N; ++n) if (s.kept(n)) m.read(n, "after forward");
        for (int n = 0; n <= s.N; ++n)                     // ... and the states of the window the header says the forward left
            if (!s.kept(n) && s.window(n) == m.resident) m.read(n, "after forward (resident window)");
        m.get(s.N, "terminal condition");
        if (cont) for (int idx = s.N; idx >= 1; --idx) m.get(idx, "continuous sweep");
        else for (int idx = s.N - 1; idx >= 0; --idx) m.get(idx, "discrete sweep");
        REQUIRE(m.replayed == expected_replays(s, cont), SCHED "%s sweep replayed %ld steps, %ld expected", SCHED_ARGS, cont ? "continuous" : "discrete", m.replayed,
                expected_replays(s, cont));
        // snapshot reads in an order that jumps between windows: a stride coprime to N + 1, then both ends inwards
        int stride = s.N / 2 + 1;
        auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
        while (gcd(stride, s.N + 1) != 1) ++stride;
        for (int i = 0; i <= s.N; ++i) m.get((int)((long)i * stride % (s.N + 1)), "snapshot read");
        for (int i = 0; i <= s.N; ++i) m.get(i & 1 ? s.N - i / 2 : i / 2, "snapshot read");
        // ... and a second gradient: forward again, sweep again, from whatever the reads left resident
        m.forward();
        m.replayed = 0;
        m.get(s.N, "terminal condition");
        for (int idx = s.N - 1; idx >= 0; --idx) m.get(idx, "second sweep");
        REQUIRE(m.replayed == expected_replays(s, 0), SCHED "second sweep replayed %ld steps", SCHED_ARGS, m.replayed);
    }
}

// ---- Poiseuille: the slot map pois.hip held before it used the shared schedule -------------------------------------------------------------
// PoisBase's members as they were, literally: one array, checkpoints first, state N, the window slots behind; slots() is the count
// tests/test_poiseuille_ckpt_gpu.py expects and include/smo.h documents
struct OldPois {
    int N, ck, n_ck;
    OldPois(int N_, int ck_) : N(N_), ck(ck_), n_ck(ck_ == 1 ? N_ + 1 : N_ / ck_ + 1) {}
    bool kept(int n) const { return ck == 1 || n % ck == 0 || n == N; }
    int slot_of(int n) const {
        if (ck == 1) return n;
        if (n % ck == 0) return n / ck;
        if (n == N) return n_ck;
        return n_ck + (N % ck != 0 ? 1 : 0) + n % ck - 1;
    }
    static size_t slots_for(int N, int k) {
        if (k == 1) return (size_t)N + 1;
        return (size_t)(N / k + 1) + (N % k != 0 ? 1 : 0) + (size_t)std::min(k - 1, N - 1);
    }
    static size_t slots(int N, int k) { return k == 1 ? N + 1 : N / k + 1 + (N % k ? 1 : 0) + std::min(k - 1, N - 1); }
    int window_after_forward() const {
        int cur_window = -1;
        for (int n = N - 1; n >= 1 && n >= N - 2; --n) if (!kept(n)) { cur_window = n / ck; break; }
        return cur_window;
    }
};
static long old_pois_slot_map() {
    long cases = 0;
    for (int N = 1; N <= 60; ++N)
        for (int ck = 1; ck <= N; ++ck, ++cases) {
            const Schedule s{N, ck, kNoDenseTail, false, true};
            const OldPois o(N, ck);
            const size_t total = s.stack_slots() + s.scratch_slots();
            REQUIRE(total == OldPois::slots_for(N, ck) && total == OldPois::slots(N, ck), SCHED "%zu slots, %zu before", SCHED_ARGS, total, OldPois::slots_for(N, ck));
            REQUIRE(s.window_after_forward() == o.window_after_forward(), SCHED "the forward solve leaves window %d, %d before", SCHED_ARGS, s.window_after_forward(),
                    o.window_after_forward());
            for (int n = 0; n <= N; ++n) {
                const Slot q = s.slot(n);
                const size_t flat = (q.scratch ? s.stack_slots() : 0) + q.index;              // PoisBase::snap
                REQUIRE(s.kept(n) == o.kept(n) && flat == (size_t)o.slot_of(n) && flat < total, SCHED "state %d kept %d in slot %zu, kept %d in slot %d before", SCHED_ARGS, n,
                        (int)s.kept(n), flat, (int)o.kept(n), o.slot_of(n));
                if (n % ck == 0) REQUIRE((size_t)(n / ck) < total, SCHED "extras record %d", SCHED_ARGS, n / ck);                        // PoisBase::ckx
                if (o.kept(n)) continue;
                const int w = n / ck, last = std::min(w * ck + ck - 1, N - 1);                // ensure_window(n / ck): restart(w ck), replay w ck .. last - 1
                REQUIRE(s.window(n) == w && s.first(w) == w * ck && s.last(w) == last, SCHED "window of state %d: %d, steps %d..%d", SCHED_ARGS, n, s.window(n), s.first(w),
                        s.last(w) - 1);
            }
        }
    REQUIRE(cases == 1830, "old slot map: %ld cases", cases);
    return cases;
}

// ---- Poiseuille: ckpt = 0 -------------------------------------------------------------------------------------------------------------------
// PoisBase::alloc_stack: the first interval in 1..N whose stack fits the bytes that may be used, else the smallest stack over k for the error text
static long pois_interval() {
    long cases = 0, none_fits = 0, one_fits = 0, least_inside = 0;
    struct Z { size_t nC, a, B; };
    const Z zs[] = {{48, 4, 1}, {2 * 13 * 24, 13, 3}, {(size_t)2 * 193 * 192, 193, 8}};
    for (const Z& z : zs)
        for (int N = 1; N <= 64; ++N) {
            const auto bytes = [&](int k) {                                                    // PoisBase::stack_bytes_for
                const Schedule s{N, k, kNoDenseTail, false, true};
                return (s.stack_slots() + s.scratch_slots()) * z.B * (3 * z.nC + (k == 1 ? 0 : 2 * z.a * 3)) * sizeof(double);
            };
            std::vector<double> budgets = {0.0, 1e30};
            for (int k = 1; k <= N; ++k) for (int d = -1; d <= 1; ++d) budgets.push_back((double)bytes(k) + d);
            for (double avail : budgets) {
                int want = 0, arg = 1;
                for (int k = N; k >= 1; --k) if ((double)bytes(k) <= avail) want = k;
                for (int k = 1; k <= N; ++k) if (bytes(k) < bytes(arg)) arg = k;
                const int got = first_interval(N, bytes, avail);
                REQUIRE(got == want, "pois interval N=%d nC=%zu B=%zu, %.0f bytes: %d, brute force %d", N, z.nC, z.B, avail, got, want);
                if (want == 0) {
                    REQUIRE(smallest_stack(N, bytes) == bytes(arg) && (double)bytes(arg) > avail, "pois interval N=%d: smallest stack %zu, brute force %zu (k = %d)", N,
                            smallest_stack(N, bytes), bytes(arg), arg);
                    ++none_fits;
                    least_inside += arg > 1 && arg < N;
                }
                one_fits += want == 1;
                ++cases;
            }
        }
    REQUIRE(none_fits > 0 && least_inside > 0 && one_fits > 0, "pois interval: %ld budgets too small (%ld with the smallest stack at 1 < k < N), %ld where k = 1 fits", none_fits,
            least_inside, one_fits);
    return cases;
}

// ---- dense tail ----------------------------------------------------------------------------------------------------------------------------
static long dense_tail() {
    long cases = 0;
    for (int N = 1; N <= 59; ++N)
        for (int ck = 2; ck <= std::min(N, 9); ++ck)
            for (int fit = 0; fit <= N + 4; ++fit, ++cases) {
                int want = kNoDenseTail;
                if (fit > N / ck + 1)
                    for (int D = 0; D <= N && want == kNoDenseTail; D += ck)
                        if (D / ck + (N - D) + 1 <= fit) want = D;
                const int got = auto_dense_from(N, ck, (size_t)fit);
                REQUIRE(got == want, "N=%d ck=%d fit=%d: dense_from %d, brute force %d", N, ck, fit, got, want);
                REQUIRE(pick_dense_from(N, ck, (size_t)fit, true, false, 0) == want, "N=%d ck=%d fit=%d: pick_dense_from", N, ck, fit);
                REQUIRE(pick_dense_from(N, ck, (size_t)fit, false, false, 0) == kNoDenseTail, "N=%d ck=%d fit=%d: tail switched off", N, ck, fit);
                if (want != kNoDenseTail) REQUIRE((Schedule{N, ck, want, false}.stack_slots() <= (size_t)fit), "N=%d ck=%d fit=%d: %d does not fit", N, ck, fit, want);
            }
    REQUIRE(cases == 16220, "dense tail: %ld cases", cases);
    return cases;
}
static long forced_tail() {
    long cases = 0;
    for (int N = 1; N <= 20; ++N)
        for (int ck = 2; ck <= std::min(N, 9); ++ck)
            for (int n = -5; n <= N + ck + 3; ++n, ++cases) {
                const int D = forced_dense_from(ck, n), c = std::max(0, n);
                REQUIRE(D % ck == 0 && D <= c && D > c - ck && D >= 0, "forced ck=%d n=%d: %d", ck, n, D);
                if (n < 0) REQUIRE(D == 0, "forced ck=%d n=%d: %d", ck, n, D);
                REQUIRE(pick_dense_from(N, ck, 0, true, true, n) == (D <= N ? D : kNoDenseTail), "forced N=%d ck=%d n=%d", N, ck, n);      // (beyond the last state: none)
            }
    return cases;
}

// ---- interval ------------------------------------------------------------------------------------------------------------------------------
static long interval() {
    long cases = 0, first_is_not_best = 0;
    const KdSizes zs[] = {{1000, 700, 900, 5000, 1, 16}, {37, 11, 5, 129, 3, 16}, {1 << 20, 3 << 20, 5 << 20, 7 << 20, 1, 16}};
    for (const KdSizes& z : zs)
        for (int N = 1; N <= 64; ++N)
            for (int T = 0; T <= N + 2; ++T)                  // free HBM: room for exactly T slots, one byte more, one byte less
                for (int d = -1; d <= 1; ++d, ++cases) {
                    const size_t free_b = (size_t)T * z.slot_bytes() + z.work_bytes() + kSpareInterval + (size_t)(d + 1) - 1;
                    int want = N, best = 1;
                    for (int k = N - 1; k >= 1; --k)
                        if ((size_t)(N / k + 1 + k - 1) * z.slot_bytes() + z.work_bytes() + kSpareInterval <= free_b) want = k;
                    for (int k = 1; k <= N; ++k) if (uniform_slots(N, k) < uniform_slots(N, best)) best = k;
                    const int got = pick_interval(N, z, free_b);
                    REQUIRE(got == want, "interval N=%d room for %d slots %+d bytes: %d, brute force %d", N, T, d, got, want);
                    REQUIRE(clamp_interval(got, N) == got && clamp_interval(N + 3, N) == N, "clamp N=%d", N);
                    if (want < N && want != best && uniform_slots(N, want) > uniform_slots(N, best)) ++first_is_not_best;
                }
    // the slot count falls up to k ~ sqrt(N) and rises again: the search returns the FIRST interval that fits, not the smallest stack
    REQUIRE(uniform_slots(64, 8) == 16 && uniform_slots(64, 32) == 34 && uniform_slots(64, 63) == 64, "slot counts past sqrt(N)");
    REQUIRE(first_is_not_best > 0, "no case where the first fitting interval is not the one with the fewest slots");
    const KdSizes z = zs[0];
    REQUIRE(pick_interval(64, z, 20 * z.slot_bytes() + z.work_bytes() + kSpareInterval) == 4, "N=64, 20 slots: interval 4 (8 would need 16 only)");
    REQUIRE(pick_interval(64, z, 15 * z.slot_bytes() + z.work_bytes() + kSpareInterval) == 64, "N=64, 15 slots: nothing fits, the search ends at N");
    return cases;
}

// ---- Ty stack and Ty cache -----------------------------------------------------------------------------------------------------------------
static long ty_buffers() {
    const KdSizes z{1000, 700, 900, 5000, 1, 16}, zb{1000, 700, 900, 5000, 4, 16};
    const int N = 50;
    const size_t stack_at = (size_t)N * z.fld * 16 + z.work_bytes() + kSpareTyStack;           // "<": one byte more than this is needed
    REQUIRE(!ty_stack_fits(N, 1, z, true, stack_at) && ty_stack_fits(N, 1, z, true, stack_at + 1), "Ty stack threshold");
    REQUIRE(!ty_stack_fits(N, 1, z, false, stack_at + 1) && !ty_stack_fits(N, 2, z, true, stack_at + 1), "Ty stack: switched off / checkpoint windows");
    REQUIRE(!ty_stack_fits(N, 1, zb, true, (size_t)1 << 50), "Ty stack: batch");
    for (const KdSizes& q : {z, zb}) {
        const size_t cache_at = (size_t)3 * q.fld * 16 * q.nbatch + q.work_bytes() + kSpareTyCache;
        REQUIRE(!ty_cache_fits(3, q, true, cache_at) && ty_cache_fits(3, q, true, cache_at + 1), "Ty cache threshold (batch %zu)", q.nbatch);
        REQUIRE(!ty_cache_fits(3, q, false, cache_at + 1) && !ty_cache_fits(1, q, true, (size_t)1 << 50), "Ty cache: switched off / every state kept");
    }
    REQUIRE(zb.work_bytes() == 4 * z.work_bytes() && zb.slot_bytes() == 4 * z.slot_bytes(), "batch factor");
    REQUIRE(z.work_bytes() == (2 * 700 + 3 * 900 + 6 * 1000) * 16 + 5000 * 8, "work bytes");
    REQUIRE(tail_ok(2, 1, 1, 0, false, false) && tail_ok(2, 1, 1, 2, true, false), "tail_ok");
    REQUIRE(!tail_ok(1, 1, 1, 0, false, false) && !tail_ok(2, 2, 1, 0, false, false) && !tail_ok(2, 1, 2, 0, false, false) && !tail_ok(2, 1, 1, 2, false, false) &&
            !tail_ok(2, 1, 1, 0, false, true), "tail_ok refusals");
    REQUIRE(dense_fit(z, kSpareDenseTail + 4 * 5000 * 8) == 0 && dense_fit(z, kSpareDenseTail + 4 * 5000 * 8 + 7 * z.slot_bytes()) == 7 && dense_fit(z, 5) == 0, "dense_fit");
    return 14;
}

// ---- the flagship: Npts = 256, 1000 steps, one GPU -------------------------------------------------------------------------------------------
// Sizes from the geometry of KDyn::init_geometry (world 1, default padding).  288 GiB is the card's nominal capacity, not a measured free
// figure: the interval is 2 for any free value between about 216 GB (below: 3) and 415 GB (above: 1), which the last four lines pin.
static long flagship() {
    const size_t Npts = 256, W = 1, ty_pad = 8, TY_KMAX = 8;
    const size_t a = Npts / 2, al = a / W, m = Npts - 1, G = 3 * Npts / 2, Gzl = G / W;
    const size_t nmode = al * m * m, tzb = 3 * al * m * Gzl, n_ex = 2 * tzb * W;
    const size_t fld = 3 * a * (G * Gzl + std::max(TY_KMAX * ty_pad, (Gzl / 8 + 1) * std::max<size_t>(ty_pad, 8)));
    const KdSizes z{nmode, n_ex, fld, 3 * G * G * Gzl, 1, 16};
    const int N = 1000;
    const int ck = pick_interval(N, z, (size_t)288 << 30);
    REQUIRE(ck == 2, "256^3 x 1000 steps, 288 GiB free: interval %d", ck);
    const Schedule s{N, 2, kNoDenseTail, false};
    const double stack_gb = 1e-9 * (double)((s.stack_slots() + s.scratch_slots()) * z.slot_bytes());
    REQUIRE(s.stack_slots() + s.scratch_slots() == 502 && uniform_slots(N, 2) == 502 && stack_gb > 200.0 && stack_gb < 201.0, "interval 2: %zu slots, %.1f GB",
            s.stack_slots() + s.scratch_slots(), stack_gb);
    REQUIRE(1e-9 * (double)(uniform_slots(N, 1) * z.slot_bytes()) > 399.0, "interval 1: about 400 GB");
    REQUIRE(pick_interval(N, z, (size_t)217e9) == 2 && pick_interval(N, z, (size_t)216e9) == 3, "lower end of interval 2");
    REQUIRE(pick_interval(N, z, (size_t)415e9) == 2 && pick_interval(N, z, (size_t)416e9) == 1, "upper end of interval 2");
    return 7;
}

// ---- tuned sizes -----------------------------------------------------------------------------------------------------------------------------
static long tuned_list() {
    const int tuned[] = {8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 60, 64, 72, 80, 96, 100, 112, 120, 128, 144, 160, 192, 200, 224, 240, 256, 320};
    long cases = 0, n = 0;
    for (int Npts = 6; Npts <= 400; Npts += 2, ++cases) {
        const bool want = std::find(std::begin(tuned), std::end(tuned), Npts) != std::end(tuned);
        REQUIRE(is_tuned(3 * Npts / 2) == want, "is_tuned(G = %d), Npts = %d", 3 * Npts / 2, Npts);
        n += is_tuned(3 * Npts / 2);
    }
    REQUIRE(n == 28, "%ld tuned sizes", n);
    return cases;
}

int main() {
    int before = fails;
    long cases = for_each_schedule(slot_map);
    group("slot map", before, cases);
    before = fails; cases = for_each_schedule(sweeps);
    group("sweeps", before, cases);
    before = fails; cases = old_pois_slot_map();
    group("old poiseuille slot map", before, cases);
    before = fails; cases = pois_interval();
    group("poiseuille interval", before, cases);
    before = fails; cases = dense_tail();
    group("dense tail", before, cases);
    before = fails; cases = forced_tail();
    group("forced tail", before, cases);
    before = fails; cases = interval();
    group("interval", before, cases);
    before = fails; cases = ty_buffers();
    group("ty buffers", before, cases);
    before = fails; cases = flagship();
    group("flagship", before, cases);
    before = fails; cases = tuned_list();
    group("tuned list", before, cases);
    if (fails) std::printf("FAIL %d checks\n", fails);
    return fails ? 1 : 0;
}
