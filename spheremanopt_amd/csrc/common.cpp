// Host plumbing of libsmo (no kernels here).
#include <cstdlib>

#include "smo_common.hpp"

namespace smo {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }

// SMO_POISON=<0..255> (tests): no allocation of the library is cleared, and a solve may rely only on what it wrote itself; with the knob set
// every block handed out is filled with that byte first, so that a read of memory nobody wrote changes the result instead of finding the
// zeros of a fresh page.  Read at every allocation (the lazy ones come long after init()); unset: this one getenv and nothing else.
int poison_byte(int* byte) {
    *byte = -1;
    const char* e = getenv("SMO_POISON");
    if (!e) return SMO_OK;
    char* end = nullptr;
    const long v = (e[0] >= '0' && e[0] <= '9') ? strtol(e, &end, 10) : -1;      // digits only: no sign, no blanks, no 0x
    if (v < 0 || v > 255 || *end != '\0') {
        set_error("SMO_POISON must be a whole number in 0..255, got \"%s\"", e);
        return SMO_ERR_ARG;
    }
    *byte = (int)v;
    return SMO_OK;
}
int poison_device(void* p, size_t bytes) {
    int byte = -1;
    SMO_TRY(poison_byte(&byte));
    if (byte < 0) return SMO_OK;
    SMO_HIP(hipMemset(p, byte, bytes));
    SMO_HIP(hipStreamSynchronize(nullptr));
    return SMO_OK;
}
int poison_host(void* p, size_t bytes) {
    int byte = -1;
    SMO_TRY(poison_byte(&byte));
    if (byte >= 0) memset(p, byte, bytes);
    return SMO_OK;
}

static const char* const kPoolSite = "DevPool::alloc";

int DevPool::alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    size_t cap = 0;
    SMO_TRY(guard_cap(&cap));
    GuardBlock b;
    hipError_t e = guard_malloc(cap, bytes, bytes, &b);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SMO_ERR_NOMEM : SMO_ERR_HIP;
    }
    int rc = guard_arm(b);
    if (rc == SMO_OK) rc = poison_device(b.ptr(), bytes);            // (the requested bytes only: slack and zones keep their pattern)
    if (rc != SMO_OK) {
        guard_free(&b);
        return rc;
    }
    *p = b.ptr();
    blocks.push_back(b);
    total += bytes;
    return SMO_OK;
}
int DevPool::free_one(void* p) {
    for (size_t i = 0; i < blocks.size(); ++i)
        if (blocks[i].ptr() == p) {
            SMO_TRY(guard_check(kPoolSite, blocks[i]));
            SMO_HIP(hipFree(blocks[i].base));
            blocks.erase(blocks.begin() + i);
            return SMO_OK;
        }
    set_error("DevPool::free_one: unknown buffer");
    return SMO_ERR_ARG;
}
int DevPool::check_live() {
    for (const GuardBlock& b : blocks) SMO_TRY(guard_check(kPoolSite, b));
    return SMO_OK;
}
void DevPool::release() {
    for (GuardBlock& b : blocks) {
        (void)guard_check(kPoolSite, b);
        guard_free(&b);
    }
    blocks.clear();
    total = 0;
}

std::vector<cplx> twiddles(int L) {
    std::vector<cplx> w(L);
    const long double two_pi = 6.283185307179586476925286766559005768L;
    for (int k = 0; k < L; ++k) {
        long double a = -two_pi * (long double)k / (long double)L;
        w[k] = mk((double)cosl(a), (double)sinl(a));
    }
    return w;
}

// ---- timing ----------------------------------------------------------------------------------------------
hipEvent_t Timing::get() {
    if (!free_ev.empty()) { hipEvent_t e = free_ev.back(); free_ev.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
void Timing::reset() {
    (void)flush();
    for (auto& c : cls) { c.launches = 0; c.total_ms = 0; }
    for (auto& n : seen) n = 0;
}
void Timing::begin(int k, hipStream_t s) {
    Pending p{k, get(), get()};
    (void)hipEventRecord(p.a, s);
    pend.push_back(p);
}
bool Timing::stamping() const {
    static const bool env_on = [] { const char* e = getenv("SMO_TIMING_STAMP"); return !(e && atoi(e) == 0); }();
    return stamp && env_on;
}
void Timing::begin_stamped(int k, hipEvent_t* a, hipEvent_t* b) {
    Pending p{k, get(), get()};
    *a = p.a; *b = p.b;
    pend.push_back(p);
}
void Timing::end(int k, hipStream_t s) {
    (void)k;
    (void)hipEventRecord(pend.back().b, s);
}
int Timing::flush() {
    for (auto& p : pend) {
        float ms = 0.f;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            cls[p.k].launches += 1;
            cls[p.k].total_ms += ms;
        }
        free_ev.push_back(p.a);
        free_ev.push_back(p.b);
    }
    pend.clear();
    return SMO_OK;
}
Timing::~Timing() {
    (void)flush();
    for (hipEvent_t e : free_ev) (void)hipEventDestroy(e);
}

// ---- context base ------------------------------------------------------------------------------------------
Context::~Context() {
    pool.release();
    if (stream && own_stream) (void)hipStreamDestroy(stream);
}

int Context::set_stream(hipStream_t s) {
    SMO_HIP(hipStreamSynchronize(stream));
    timing.flush();
    if (stream && own_stream) (void)hipStreamDestroy(stream);
    stream = s;
    own_stream = false;
    return SMO_OK;
}

int Context::base_init() {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_error("no usable HIP device (%s); libsmo has no CPU fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return SMO_ERR_NO_DEVICE;
    }
    if (cfg.device < 0 || cfg.device >= ndev) {
        set_error("device %d out of range (have %d)", cfg.device, ndev);
        return SMO_ERR_ARG;
    }
    SMO_HIP(hipSetDevice(cfg.device));
    SMO_TRY(lds_poison_read());                                      // SMO_POISON_LDS: read here and in pool_for, tested at every launch
    SMO_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return SMO_OK;
}

int Context::forward_host(const double* const* X, double* J) {
    SMO_HIP(hipSetDevice(cfg.device));
    const size_t bytes = vec_len * (size_t)cfg.batch * sizeof(double);
    for (int c = 0; c < n_comp; ++c) {
        if (!stage_x[c]) SMO_TRY(pool.alloc(&stage_x[c], vec_len * (size_t)cfg.batch));
        SMO_HIP(hipMemcpyAsync(stage_x[c], X[c], bytes, hipMemcpyHostToDevice, stream));
    }
    return forward_dev(stage_x, J);
}

int Context::adjoint_host(const double* const* X, int adjoint_type, double* const* grad) {
    SMO_HIP(hipSetDevice(cfg.device));
    const size_t bytes = vec_len * (size_t)cfg.batch * sizeof(double);
    for (int c = 0; c < n_comp; ++c) {
        if (!stage_x[c]) SMO_TRY(pool.alloc(&stage_x[c], vec_len * (size_t)cfg.batch));
        if (c < n_grads() && !stage_g[c]) SMO_TRY(pool.alloc(&stage_g[c], vec_len * (size_t)cfg.batch));
        if (X && X[c]) SMO_HIP(hipMemcpyAsync(stage_x[c], X[c], bytes, hipMemcpyHostToDevice, stream));
    }
    SMO_TRY(adjoint_dev(stage_x, adjoint_type, stage_g));
    for (int c = 0; c < n_grads(); ++c) SMO_HIP(hipMemcpyAsync(grad[c], stage_g[c], bytes, hipMemcpyDeviceToHost, stream));
    SMO_HIP(hipStreamSynchronize(stream));
    return SMO_OK;
}

int Context::hessvec_host(const double* const* V, double* const* HV, double* dJ) {
    SMO_HIP(hipSetDevice(cfg.device));
    const size_t n = vec_len * (size_t)cfg.batch;
    for (int c = 0; c < 2; ++c)
        if (!stage_hv[c]) SMO_TRY(pool.alloc(&stage_hv[c], n));
    SMO_HIP(hipMemcpyAsync(stage_hv[0], V[0], n * sizeof(double), hipMemcpyHostToDevice, stream));
    SMO_TRY(hessvec_dev(stage_hv, stage_hv + 1, dJ));
    SMO_HIP(hipMemcpyAsync(HV[0], stage_hv[1], n * sizeof(double), hipMemcpyDeviceToHost, stream));
    SMO_HIP(hipStreamSynchronize(stream));
    return SMO_OK;
}

int Context::inner_host(const double* x, const double* y, double* out) {
    SMO_HIP(hipSetDevice(cfg.device));
    const size_t n = vec_len * (size_t)cfg.batch;
    for (int c = 0; c < 2; ++c)
        if (!stage_g[c]) SMO_TRY(pool.alloc(&stage_g[c], n));
    SMO_HIP(hipMemcpyAsync(stage_g[0], x, n * sizeof(double), hipMemcpyHostToDevice, stream));
    SMO_HIP(hipMemcpyAsync(stage_g[1], y, n * sizeof(double), hipMemcpyHostToDevice, stream));
    return inner_dev(stage_g[0], stage_g[1], out);
}

}  // namespace smo
