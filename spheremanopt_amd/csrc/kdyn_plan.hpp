// Host side of the KDYN context that is pure integer arithmetic (kdyn.hip: class KDyn): what a context may take from the free HBM and which
// transform lengths have tuned kernels.  Which forward state lives in which slot of the snapshot stack is ckpt::Schedule of ckpt_plan.hpp,
// the schedule the Poiseuille contexts share (there with keep_last: state N always kept, never written by a replay); KDyn's has a dense tail
// or ping-pong slots instead, both chosen below.
//
// Host-only: no HIP type is named here (sizes enter as byte counts), so g++ alone compiles it and tests/c/kdyn_plan_test.cpp walks every
// schedule on the CPU (tests/test_kdyn_plan.py).  KDyn::init() asks hipMemGetInfo between its allocations and hands each figure to one of the
// functions below; nothing here allocates or launches.
#pragma once
#include <algorithm>
#include <cstddef>

#include "ckpt_plan.hpp"

namespace smo {
namespace kdplan {

// ---- what a context takes from the free HBM --------------------------------------------------------------------------------------------
// Element counts of the context's buffers (KDyn::init_geometry) and the bytes of one complex element.
struct KdSizes {
    size_t nmode, n_ex, fld, n_grid;          // one member: modes per component, an exchange buffer, a field group of Ty, a grid vector
    size_t nbatch, cplx;
    size_t slot_bytes() const { return nbatch * 3 * nmode * cplx; }                                         // one snapshot, every member
    size_t work_bytes() const { return nbatch * ((2 * n_ex + 3 * fld + 6 * nmode) * cplx + n_grid * 8); }   // the buffers allocated after the stack
};
// HBM left free beyond the work buffers by each decision
constexpr size_t kSpareInterval = (size_t)8 << 30;       // ckpt = 0: the interval
constexpr size_t kSpareTyStack = (size_t)16 << 30;       // the grid-side stack of the forward states
constexpr size_t kSpareTyCache = (size_t)6 << 30;        // the Ty cache of the window being replayed
constexpr size_t kSpareDenseTail = (size_t)12 << 30;     // the dense tail (+ the staging vectors of the host-buffer entry points)

// slots of a uniform schedule of interval k: stack and scratch window
inline size_t uniform_slots(int N, int k) { return (size_t)N / k + 1 + (size_t)(k - 1); }
// ckpt = 0: the first interval whose slots fit the free HBM beside the work buffers; N when none does (the count falls up to k ~ sqrt(N) and
// rises again beyond: the first that fits, not the smallest stack)
inline int pick_interval(int N, const KdSizes& z, size_t free_b) {
    const int fits = ckpt::first_interval(N, [&](int k) { return uniform_slots(N, k) * z.slot_bytes() + z.work_bytes() + kSpareInterval; }, free_b);
    return fits ? fits : N;
}
inline int clamp_interval(int ck, int N) { return ck > N ? N : ck; }
// A dense tail: checkpoint windows on ONE GPU, one problem; with slabs the ranks would have to agree on the tail as they do on the interval.
// An explicit interval (smo_config.ckpt > 1) is kept as asked for unless SMO_KD_DENSE_FROM names a tail: the automatic tail belongs to ckpt = 0.
inline bool tail_ok(int ck, int world, int batch, int cfg_ckpt, bool dense_from_set, bool force_exchange) {
    return ck > 1 && world == 1 && batch == 1 && (cfg_ckpt == 0 || dense_from_set) && !force_exchange;
}
// Ty stack: only when every snapshot is kept (one problem) and kSpareTyStack stays free afterwards
// (reached with batch 1 only, where the batch factor of work_bytes is 1: the test it replaces carried none)
inline bool ty_stack_fits(int N, int ck, const KdSizes& z, bool enabled, size_t free_b) {
    return ck == 1 && z.nbatch == 1 && enabled && (size_t)N * z.fld * z.cplx + z.work_bytes() + kSpareTyStack < free_b;
}
inline bool ty_cache_fits(int ck, const KdSizes& z, bool enabled, size_t free_b) {
    return ck > 1 && enabled && (size_t)ck * z.fld * z.cplx * z.nbatch + z.work_bytes() + kSpareTyCache < free_b;
}
// snapshots (one problem) that fit the HBM free once everything but the stack is allocated
inline size_t dense_fit(const KdSizes& z, size_t free_b) {
    const size_t keep = kSpareDenseTail + 4 * z.n_grid * sizeof(double);
    return free_b > keep ? (free_b - keep) / (3 * z.nmode * z.cplx) : 0;
}
// first dense index for `fit` snapshots: the smallest multiple D of ck in [0, N] with slots(D) = D / ck + (N - D) + 1 <= fit; none when the
// uniform stack is all that fits
inline int auto_dense_from(int N, int ck, size_t fit) {
    const long base_slots = N / ck + 1, extra = (long)fit - base_slots;
    if (extra <= 0) return ckpt::kNoDenseTail;
    const long need = (long)N + 1 - base_slots - extra;              // = D (1 - 1/ck) at least
    long D = need <= 0 ? 0 : (need * ck + (ck - 2)) / (ck - 1);
    D = (D + ck - 1) / ck * ck;
    return D <= N ? (int)D : ckpt::kNoDenseTail;
}
// SMO_KD_DENSE_FROM = n: rounded down to a multiple of the interval
inline int forced_dense_from(int ck, int n) { return std::max(0, n) / ck * ck; }
// the tail of a context with tail_ok: forced, else automatic unless switched off (SMO_KD_DENSE_TAIL=0); beyond the last state = none
inline int pick_dense_from(int N, int ck, size_t fit, bool automatic, bool forced, int forced_n) {
    const int df = forced ? forced_dense_from(ck, forced_n) : (automatic ? auto_dense_from(N, ck, fit) : ckpt::kNoDenseTail);
    return df <= N ? df : ckpt::kNoDenseTail;
}

// ---- tuned transform lengths -----------------------------------------------------------------------------------------------------------
// G = 3 Npts / 2 with factors 2, 3, 5 and 7 for which kdyn.hip instantiates its kernels (KDyn::with_L is generated from this list, in this
// order); every other even Npts runs the run-time-length kernels of kdyn_any.hpp.
#define SMO_KD_TUNED_G(X)                                                                                        \
    X(12) X(24)                                                                                                  \
    X(30) X(60) X(120) X(240) X(480)        /* Npts = 20, 40, 80, 160, 320: one radix-5 stage */                 \
    X(90) X(180) X(360) X(150) X(300)       /* Npts = 60, 120, 240 and 100, 200: factors 3 and 5 together, 5 twice */ \
    X(42) X(84) X(168) X(336)               /* Npts = 28, 56, 112, 224: one radix-7 stage */                     \
    X(18) X(54) X(108) X(216)               /* Npts = 12, 36, 72, 144: 3 more than once */                       \
    X(36) X(72) X(144)                      /* Npts = 24, the reference script's default */                      \
    X(48) X(96) X(192) X(288) X(384)
inline bool is_tuned(int G) {
    switch (G) {
#define SMO_KD_CASE(L) case L:
        SMO_KD_TUNED_G(SMO_KD_CASE)
#undef SMO_KD_CASE
        return true;
    }
    return false;
}

}  // namespace kdplan
}  // namespace smo
