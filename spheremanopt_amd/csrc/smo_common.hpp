// Shared host-side plumbing of libsmo: error reporting, device buffers, the context base class and
// HIP-event kernel timing.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smo.h"
#include "guard.hpp"
#include "lds_poison.hpp"

namespace smo {

// ---------------------------------------------------------------------------------------------------------
// complex128 as a plain 16-byte pair (one ds_read_b128 / global_load_dwordx4 per element)
// ---------------------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) cplx {
    double re, im;
};
__host__ __device__ inline cplx mk(double r, double i) { cplx c; c.re = r; c.im = i; return c; }
__host__ __device__ inline cplx operator+(cplx a, cplx b) { return mk(a.re + b.re, a.im + b.im); }
__host__ __device__ inline cplx operator-(cplx a, cplx b) { return mk(a.re - b.re, a.im - b.im); }
__host__ __device__ inline cplx operator*(cplx a, cplx b) { return mk(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
__host__ __device__ inline cplx operator*(double s, cplx a) { return mk(s * a.re, s * a.im); }
__host__ __device__ inline cplx conj(cplx a) { return mk(a.re, -a.im); }
__host__ __device__ inline cplx mul_i(cplx a) { return mk(-a.im, a.re); }        //  i * a
__host__ __device__ inline cplx mul_mi(cplx a) { return mk(a.im, -a.re); }       // -i * a
__host__ __device__ inline cplx mul_conj(cplx a, cplx w) {                       //  a * conj(w)
    return mk(a.re * w.re + a.im * w.im, a.im * w.re - a.re * w.im);
}

// ---------------------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
const char* last_error();

#define SMO_HIP(call)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            smo::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SMO_ERR_HIP;                                                                    \
        }                                                                                          \
    } while (0)

#define SMO_TRY(expr)                 \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != SMO_OK) return rc_; \
    } while (0)

// ---------------------------------------------------------------------------------------------------------
// environment knobs: each context declares its own in ONE struct (KDynEnv, PoisEnv, ShbEnv, ShEnv) and reads them once, in init()
// ---------------------------------------------------------------------------------------------------------
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline double env_double(const char* name, double dflt) { const char* e = getenv(name); return e ? atof(e) : dflt; }
inline std::string env_str(const char* name) { const char* e = getenv(name); return e ? e : ""; }     // unset and empty both give "": pair with env_set
inline bool env_on(const char* name) { return env_int(name, 1) != 0; }       // default-on flag: NAME=0 switches it off
inline bool env_is1(const char* name) { return env_int(name, 0) == 1; }      // default-off flag: NAME=1 switches it on

// SMO_POISON=<0..255>: fill a block that is about to be handed out with that byte and wait for the fill (unset: one getenv, nothing else;
// anything but a whole number in 0..255: SMO_ERR_ARG).  Read at the allocation, not in init().  The one helper of every device allocation
// site (DevPool::alloc, smo_vec_alloc), and its host twin for smo_host_alloc.
int poison_device(void* p, size_t bytes);
int poison_host(void* p, size_t bytes);

// SMO_GUARD=<cap in bytes> (tests; guard.hpp, guard.hip): with the knob set a device block lies between two zones of a known pattern, which
// are compared when the block is given back; smo_guard_report adds the results up.  Unset: one getenv per allocation, the plain hipMalloc.
// Whether a block is guarded is kept with the block, so a knob that changes later does not matter.
struct GuardBlock {
    void* base = nullptr;            // what hipMalloc returned
    size_t requested = 0, zone = 0;  // zone == 0: not guarded, base is the pointer handed out
    int device = 0;
    bool guarded() const { return zone != 0; }
    guard::Layout layout() const { guard::Layout l; l.requested = requested; l.zone = zone; return l; }
    void* ptr() const { return static_cast<char*>(base) + zone; }
};
int guard_cap(size_t* cap);                                      // THE reader of SMO_GUARD: 0 when unset, SMO_ERR_ARG for a bad value
hipError_t guard_malloc(size_t cap, size_t requested, size_t plain_bytes, GuardBlock* b);      // cap == 0: hipMalloc(plain_bytes) and nothing else
int guard_arm(const GuardBlock& b);                              // pattern zones and slack, wait for it (not guarded: nothing)
int guard_check(const char* site, const GuardBlock& b);          // wait for the device, compare, add to the tally, pattern a damaged block again
void guard_free(GuardBlock* b);
void guard_take(size_t* checked, size_t* damaged, char* first, size_t first_len);      // read and reset the tally
int vec_guard_check_all();                                       // vecops.hip: the live and the pooled device vectors of every device

// device allocation that records itself for release in the context destructor
struct DevPool {
    std::vector<GuardBlock> blocks;      // ptr(): what was handed out; base: what hipFree gets (the same unless SMO_GUARD was set)
    size_t total = 0;
    int check_live();                    // smo_guard_report: compare the zones of every block now (the caller has drained the context)
    int alloc(void** p, size_t bytes);
    template <class T> int alloc(T** p, size_t n) { return alloc(reinterpret_cast<void**>(p), n * sizeof(T)); }
    template <class T> int upload(T** p, const std::vector<T>& h, hipStream_t s) {
        SMO_TRY(alloc(p, h.size()));
        SMO_HIP(hipMemcpyAsync(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
        SMO_HIP(hipStreamSynchronize(s));
        return SMO_OK;
    }
    int free_one(void* p);              // give one buffer back before the context goes away
    void release();
};

// exp(-2 pi i k / L), k = 0..L-1, evaluated in long double
std::vector<cplx> twiddles(int L);

// ---------------------------------------------------------------------------------------------------------
// kernel timing: one accumulator per kernel class, HIP events recorded on the context's stream
// ---------------------------------------------------------------------------------------------------------
struct TimingClass {
    std::string name;
    double bytes_per_launch = 0;     // algorithmic bytes of ONE launch (every axis pass of every field reads + writes HBM)
    long long launches = 0;
    double total_ms = 0;
    double hbm_bytes = 0;            // compulsory HBM bytes of ONE launch of the kernel AS FUSED: each input read once,
                                     // each output written once; <= bytes_per_launch, and what the roofline fraction is taken against
};

class Timing {
public:
    bool on = false;
    unsigned long long mask = ~0ull;  // classes whose launches are timed (bit k = class k): keeps the event overhead out of the other launches
    int stride = 1;                   // of a selected class, every stride-th launch is timed (smo_timing_stride): a uniform sample at 1/stride of the event cost
    // How a timed launch gets its interval.  stamp = true (default; SMO_TIMING_STAMP=0 disables): the launch goes through
    // hipExtLaunchKernelGGL(..., startEvent, stopEvent), whose events carry the dispatch's OWN begin / end timestamps — the quantity
    // rocprofv3 --kernel-trace reports — and put no marker packet into the queue.  stamp = false (and every class that is not a single
    // kernel launch, e.g. the exchanges): hipEventRecord before and after, i.e. two marker packets; a start marker recorded straight behind
    // an un-timed kernel is processed while that kernel's last workgroups still run, so such an interval includes the predecessor's tail
    // (round 3: the every-8th-launch sample read 2.4-4.6 % above the every-launch average).
    bool stamp = true;
    std::vector<long long> seen;      // launches of each class since the last reset, timed or not
    std::vector<TimingClass> cls;
    int add_class(const char* name, double bytes, double hbm = -1.0) {
        cls.push_back({name, bytes, 0, 0.0, hbm < 0 ? bytes : hbm});
        seen.push_back(0);
        return (int)cls.size() - 1;
    }
    void reset();
    void begin(int k, hipStream_t s);
    void end(int k, hipStream_t s);
    bool stamping() const;            // stamp && !SMO_TIMING_STAMP=0
    void begin_stamped(int k, hipEvent_t* a, hipEvent_t* b);      // events for hipExtLaunchKernelGGL; nothing is recorded here
    int flush();                      // resolve pending event pairs (after a stream sync)
    ~Timing();
private:
    struct Pending { int k; hipEvent_t a, b; };
    std::vector<Pending> pend;
    std::vector<hipEvent_t> free_ev;
    hipEvent_t get();
};

struct ScopedTimer {
    Timing& t; int k; hipStream_t s;
    bool active;
    bool stamped = false;             // the launch itself carries the events (SMO_LAUNCH_T): no markers
    hipEvent_t ea = nullptr, eb = nullptr;
    ScopedTimer(Timing& t_, int k_, hipStream_t s_, bool single_kernel = false)
        : t(t_), k(k_), s(s_), active(t_.on && k_ >= 0 && k_ < 64 && ((t_.mask >> k_) & 1ull)) {
        if (active && t.stride > 1) active = (t.seen[k]++ % t.stride) == 0;
        if (active && single_kernel && t.stamping()) { stamped = true; t.begin_stamped(k, &ea, &eb); }
        else if (active) t.begin(k, s);
    }
    ~ScopedTimer() { if (active && !stamped) t.end(k, s); }
};
// ---------------------------------------------------------------------------------------------------------
// THE launch hook: every kernel launch of the library is one of the three macros below, and no other file names a launch primitive
// (tests/test_lds_poison_cpu.py).
//
// SMO_POISON_LDS=<0..255> (tests; lds_poison.hip): LDS is not cleared between dispatches, so a workgroup starts with what the last
// workgroup on its CU left behind — in a test process the previous kernel of the same solve.  With the knob set every launch is preceded,
// on the same stream (inside a capture: as a node of the same graph), by a fill dispatch that leaves that byte in every byte of every CU's
// LDS.  The knob is read by lds_poison_read() where a context is created (Context::base_init) and where the vector pool is entered
// (pool_for), never at a launch; what the hook tests is the process-wide value of the last read (-1: unset).  Unset, a launch costs this
// one relaxed load and branch.
// ---------------------------------------------------------------------------------------------------------
extern std::atomic<int> g_lds_poison;                            // the byte of the last lds_poison_read(), -1 when the knob was unset then
int lds_poison_read();                                           // THE reader of SMO_POISON_LDS; readies the current device for the fill
void lds_fill(hipStream_t s);                                    // the fill dispatch on s (current device); counts itself and the launch it precedes
void lds_take(size_t* fills, size_t* launches);                  // read and reset the two counters
inline void lds_before_launch(hipStream_t s) {
    if (g_lds_poison.load(std::memory_order_relaxed) >= 0) lds_fill(s);
}
// SMO_LAUNCH_BEGIN
#define SMO_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                                         \
    do {                                                                                                                            \
        smo::lds_before_launch(stream);                                                                                             \
        hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                                        \
    } while (0)
// launch `kernel` under ScopedTimer `tm` (constructed with single_kernel = true): with the dispatch's own timestamps when it is a timed launch
// (the fill goes first, outside the stamped interval)
#define SMO_LAUNCH_T(tm, kernel, grid, block, shmem, stream, ...)                                                                   \
    do {                                                                                                                            \
        smo::lds_before_launch(stream);                                                                                             \
        if ((tm).stamped) hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, (tm).ea, (tm).eb, 0, __VA_ARGS__);               \
        else hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                                  \
    } while (0)
// the fill dispatch itself, and nothing else: the one launch that is not preceded by a fill
#define SMO_LAUNCH_THE_FILL(kernel, grid, block, shmem, stream, ...) hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__)
// SMO_LAUNCH_END

// ---------------------------------------------------------------------------------------------------------
// context base
// ---------------------------------------------------------------------------------------------------------
class Context {
public:
    smo_config cfg{};
    hipStream_t stream = nullptr;
    bool own_stream = true;
    DevPool pool;
    Timing timing;
    bool have_forward = false;
    int n_comp = 1;
    size_t vec_len = 0;          // doubles per component per batch member
    size_t stack_bytes = 0;
    size_t snapshot_doubles = 0;
    // smo_create_members: one parameter value per batch member (KDYN: Rm, SH23: a), set between the factory and init(); empty for every
    // other context, whose members share cfg.param
    std::vector<double> member_params;
    // smo_create_frozen_u (KDYN): the velocity is given, only dJ/dB0 is asked for; keep_states = false: no snapshot stack either (Final cost).
    // Set between the factory and init() like member_params.
    bool frozen_u = false, keep_states = true;
    // smo_set_horizons: one number of steps per batch member, each in [1, cfg.n_iters] (cfg.n_iters stays the capacity everything is sized for);
    // empty: none set, every member runs cfg.n_iters steps.  check_horizons says whether this context takes them at all, set_horizons receives
    // values that are already range-checked (null: remove them).
    std::vector<int> horizons;
    virtual int check_horizons() {
        set_error("smo_set_horizons: this context runs every member for cfg.n_iters steps (members with their own horizon: KDYN on one GPU, SH23)");
        return SMO_ERR_UNSUPPORTED;
    }
    virtual int set_horizons(const int* n_iters) { (void)n_iters; return SMO_ERR_UNSUPPORTED; }

    // Cross-member block operations (csrc/blockops.hip; smo_gram*, smo_combine*): the Gram matrix <x_a, y_b> / block_scale() and the
    // recombination out_b = sum_a C[a][b] x_a on the [batch][vec_len] vectors of a batched context.  block_scale() is the divisor of the
    // context's UNWEIGHTED inner product — KDYN on one GPU: G^3 = vec_len / 3 (Inner_Prod_3), SH23: G = vec_len — and 0 where the context
    // refuses them (SHB23, POIS: weighted inner products; slabs and multi-device contexts: distributed vectors).  The factory registers the
    // kernels' timing classes behind the context's own (block_register, after init()).
    double block_scale() const;
    struct BlockOps {
        double* d_partial = nullptr;     // [workgroup][batch][batch] partial Gram blocks
        size_t partial_len = 0;
        double* d_out = nullptr;         // [batch][batch]
        double* d_C = nullptr;           // the coefficients of smo_combine*, columns padded to the kernel's register tile
        std::vector<double> h_C;
        int k_gram_xx = -1, k_gram_xy = -1, k_combine = -1;
    } bo;
    int block_register();
    int block_check(const char* who);
    int gram_dev(const double* x, const double* y, double* out_host);
    int combine_dev(const double* C_host, const double* x, double* out);
    int gram_host(const double* x, const double* y, double* out);
    int combine_host(const double* C_host, const double* x, double* out);

    virtual ~Context();
    virtual int init() = 0;
    virtual int forward_dev(const double* const* X, double* J_host) = 0;
    virtual int adjoint_dev(const double* const* X, int adjoint_type, double* const* grad) = 0;
    virtual int inner_dev(const double* x, const double* y, double* out_host) = 0;
    // smo_hessvec*: H.V of the discrete cost at the point of the last forward solve, and the directional derivative (dJ_host may be null).
    // check_hessvec says whether this context has the product at all (SH23 alone); hessvec_host stages through two vectors of its own.
    virtual int check_hessvec() {
        set_error("smo_hessvec: this problem kind has no Hessian-vector product (SH23 alone: the tangent and second-order adjoint sweeps of csrc/sh23_hessvec.hpp)");
        return SMO_ERR_UNSUPPORTED;
    }
    virtual int hessvec_dev(const double* const* V, double* const* HV, double* dJ_host) { (void)V; (void)HV; (void)dJ_host; return check_hessvec(); }
    int hessvec_host(const double* const* V, double* const* HV, double* dJ_host);
    // <x,y> of vectors given slab by slab (one pointer per device of a multi-device context; a plain context has one slab: the vector)
    virtual int inner_slabs(const double* const* x, const double* const* y, double* out_host) { return inner_dev(x[0], y[0], out_host); }
    virtual int snapshot_read(int b, int index, double* out) = 0;
    virtual int transform_host(int which, const double* in, double* out) {
        (void)which; (void)in; (void)out;
        set_error("smo_transform: not available for this problem kind");
        return SMO_ERR_UNSUPPORTED;
    }

    virtual double info(int key) const { return key == 0 ? 1.0 : 0.0; }
    virtual int kdyn_op(int op, int i0, int i1, void* p0, void* p1, double* out) {
        (void)op; (void)i0; (void)i1; (void)p0; (void)p1; (void)out;
        set_error("smo_kdyn_op: not a KDYN context");
        return SMO_ERR_UNSUPPORTED;
    }
    // slab communicator (KDYN with world > 1): see include/smo.h "in-library time loop"
    virtual int comm_init(const void* id128) { (void)id128; set_error("smo_comm_init: not a KDYN context"); return SMO_ERR_UNSUPPORTED; }
    virtual int comm_set_transport(smo_alltoall_fn a2a, smo_allreduce_fn ared, void* user) {
        (void)a2a; (void)ared; (void)user;
        set_error("smo_comm_set_transport: not a KDYN context");
        return SMO_ERR_UNSUPPORTED;
    }
    virtual double comm_info(int key) const { (void)key; return 0.0; }
    // ranks of ONE process (smo_create_multi): the context becomes rank `rank` of the group; collective like comm_init
    virtual int comm_set_peers(class PeerGroup* g, int rank) { (void)g; (void)rank; set_error("multi-device contexts: KDYN only"); return SMO_ERR_UNSUPPORTED; }
    virtual int set_stream(hipStream_t s);      // run on a caller-owned stream (e.g. torch's current stream) instead of the private one
    // device pointers the _dev entry points dereference (a multi-device context: one slab per component and device), slabs of smo_inner_slabs
    virtual int n_dev_ptrs() const { return n_comp; }
    // gradient vectors smo_adjoint[_dev] fills (a frozen-velocity KDYN context: the first one only, the second pointer may be null)
    virtual int n_grads() const { return n_comp; }
    virtual int n_slabs() const { return 1; }

    // host-buffer variants: stage through context-owned device vectors (a multi-device context scatters / gathers slabs instead)
    virtual int forward_host(const double* const* X, double* J);
    virtual int adjoint_host(const double* const* X, int adjoint_type, double* const* grad);
    virtual int inner_host(const double* x, const double* y, double* out);
    // the kernel timing behind smo_timing_* (a multi-device context answers with rank 0's) and a wait for everything enqueued
    virtual Timing& tm() { return timing; }
    virtual int sync_all() { SMO_HIP(hipSetDevice(cfg.device)); SMO_HIP(hipStreamSynchronize(stream)); return SMO_OK; }
    // smo_guard_report: drain the context and check the guard zones of every live block of its pool (a multi-device context: of every rank's)
    virtual int guard_check_live() { SMO_TRY(sync_all()); return pool.check_live(); }

protected:
    int base_init();             // device selection, stream, staging buffers (needs n_comp / vec_len set)
    double* stage_x[2] = {nullptr, nullptr};
    double* stage_g[2] = {nullptr, nullptr};
    double* stage_hv[2] = {nullptr, nullptr};      // hessvec_host: V and H.V (the forward input stays in stage_x)
};

Context* make_sh23(const smo_config& cfg);
Context* make_shb23(const smo_config& cfg);
Context* make_kdyn(const smo_config& cfg);
Context* make_pois(const smo_config& cfg);
// one context that slab-decomposes a KDYN problem over several GPUs of this process (csrc/multi.cpp)
Context* make_multi(const smo_config& cfg, int ndev, const int* dev_ids);

}  // namespace smo
