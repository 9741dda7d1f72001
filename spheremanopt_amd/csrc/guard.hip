// SMO_GUARD (tests): guard zones around every device allocation of the library, patterned and compared on the device.  Rule, pattern and
// comparison: guard.hpp (host-only, checked on the CPU); here the one reader of the knob, the two kernels and the process-wide tally
// behind smo_guard_report (capi.cpp).  Both device allocation sites (DevPool::alloc in common.cpp, smo_vec_alloc in vecops.hip) go through
// guard_malloc / guard_arm / guard_check / guard_free and keep a GuardBlock per block; with the knob unset a GuardBlock is the plain
// hipMalloc pointer.
#include <algorithm>
#include <mutex>
#include <string>

#include "smo_common.hpp"

namespace smo {
namespace {

// one launch for both regions: word w < nf is front word w, else word w - nf of the tail (slack + back zone)
__global__ __launch_bounds__(256) void guard_fill_kernel(uint64_t* front, size_t nf, uint64_t* tail, size_t nt, unsigned skip) {
    for (size_t w = blockIdx.x * (size_t)256 + threadIdx.x; w < nf + nt; w += (size_t)gridDim.x * 256) {
        if (w < nf) front[w] = guard::word(guard::FRONT, w);
        else {
            const size_t i = w - nf;
            tail[i] = (i == 0 && skip) ? guard::merged(guard::TAIL, 0, skip, tail[0]) : guard::word(guard::TAIL, i);
        }
    }
}

// res[0] += damaged words, res[1] = min(first damaged byte of the front zone), res[2] = the same of the tail: integer atomics only, and
// only from a lane that found damage
__global__ __launch_bounds__(256) void guard_count_kernel(const uint64_t* front, size_t nf, const uint64_t* tail, size_t nt, unsigned skip,
                                                          unsigned long long* res) {
    for (size_t w = blockIdx.x * (size_t)256 + threadIdx.x; w < nf + nt; w += (size_t)gridDim.x * 256) {
        const bool fr = w < nf;
        const size_t i = fr ? w : w - nf;
        const unsigned bad = guard::first_bad_byte(fr ? guard::FRONT : guard::TAIL, i, (!fr && i == 0) ? skip : 0, fr ? front[i] : tail[i]);
        if (bad < 8) {
            atomicAdd(&res[0], 1ull);
            atomicMin(&res[fr ? 1 : 2], (unsigned long long)(8 * i + bad));
        }
    }
}

struct Tally {
    std::mutex mu;
    size_t checked = 0, damaged = 0;
    std::string first;
} g_tally;

unsigned grid_for(size_t words) { return (unsigned)std::min<size_t>(4096, (words + 255) / 256); }

// the device the block lives on, for the length of one check or fill (smo_vec_free and the report do not run on the caller's device)
struct OnDevice {
    int before = -1;
    bool moved = false;
    explicit OnDevice(int device) {
        if (hipGetDevice(&before) == hipSuccess && before != device) moved = hipSetDevice(device) == hipSuccess;
    }
    ~OnDevice() { if (moved) (void)hipSetDevice(before); }
};

}  // namespace

int guard_cap(size_t* cap) {
    *cap = 0;
    const char* e = getenv("SMO_GUARD");
    if (!e) return SMO_OK;
    if (!guard::parse_cap(e, cap)) {
        set_error("SMO_GUARD must be a whole number of bytes, a multiple of 256 in 4096 .. 1073741824, got \"%s\"", e);
        return SMO_ERR_ARG;
    }
    return SMO_OK;
}

hipError_t guard_malloc(size_t cap, size_t requested, size_t plain_bytes, GuardBlock* b) {
    *b = GuardBlock();
    b->requested = requested;
    if (cap == 0) return hipMalloc(&b->base, plain_bytes);
    b->zone = guard::zone_bytes(requested, cap);
    (void)hipGetDevice(&b->device);
    const hipError_t e = hipMalloc(&b->base, b->layout().total());
    if (e != hipSuccess) b->zone = 0;
    return e;
}

void guard_free(GuardBlock* b) {
    if (b->base) (void)hipFree(b->base);
    *b = GuardBlock();
}

int guard_arm(const GuardBlock& b) {
    if (!b.guarded()) return SMO_OK;
    OnDevice dev(b.device);
    const guard::Layout l = b.layout();
    char* base = static_cast<char*>(b.base);
    const size_t nf = l.front_words(), nt = l.tail_words();
    SMO_LAUNCH(guard_fill_kernel, dim3(grid_for(nf + nt)), dim3(256), 0, nullptr, reinterpret_cast<uint64_t*>(base), nf,
                       reinterpret_cast<uint64_t*>(base + l.tail()), nt, l.tail_skip());
    SMO_HIP(hipGetLastError());
    SMO_HIP(hipStreamSynchronize(nullptr));
    return SMO_OK;
}

int guard_check(const char* site, const GuardBlock& b) {
    if (!b.guarded()) return SMO_OK;
    OnDevice dev(b.device);
    const guard::Layout l = b.layout();
    char* base = static_cast<char*>(b.base);
    unsigned long long* res = reinterpret_cast<unsigned long long*>(base + l.result());
    const size_t nf = l.front_words(), nt = l.tail_words();
    SMO_HIP(hipDeviceSynchronize());                               // the work that used the block has drained
    SMO_HIP(hipMemsetAsync(res, 0, 8, nullptr));
    SMO_HIP(hipMemsetAsync(res + 1, 0xFF, 16, nullptr));
    SMO_LAUNCH(guard_count_kernel, dim3(grid_for(nf + nt)), dim3(256), 0, nullptr, reinterpret_cast<const uint64_t*>(base), nf,
                       reinterpret_cast<const uint64_t*>(base + l.tail()), nt, l.tail_skip(), res);
    SMO_HIP(hipGetLastError());
    unsigned long long h[3] = {0, 0, 0};
    SMO_HIP(hipMemcpy(h, res, sizeof(h), hipMemcpyDeviceToHost));
    std::string line;
    if (h[0] != 0) {
        guard::Damage front, tail;
        if (h[1] != ~0ull) { front.words = 1; front.first = (size_t)h[1]; }
        if (h[2] != ~0ull) { tail.words = 1; tail.first = (size_t)h[2]; }
        const guard::Where w = guard::where(l, front, tail);
        char buf[256];
        snprintf(buf, sizeof(buf), "%s, %zu bytes requested: %s, first damaged byte at %s%+lld, %llu damaged 8-byte word(s)", site, b.requested,
                 w.zone, w.from_start ? "start" : "end", w.offset, h[0]);
        line = buf;
    }
    {
        std::lock_guard<std::mutex> lk(g_tally.mu);
        g_tally.checked += 1;
        if (h[0] != 0) {
            if (g_tally.damaged == 0) g_tally.first = line;
            g_tally.damaged += 1;
        }
    }
    // a damaged zone is patterned again: the next check reports what was stored since this one
    return h[0] != 0 ? guard_arm(b) : SMO_OK;
}

void guard_take(size_t* checked, size_t* damaged, char* first, size_t first_len) {
    std::lock_guard<std::mutex> lk(g_tally.mu);
    if (checked) *checked = g_tally.checked;
    if (damaged) *damaged = g_tally.damaged;
    if (first && first_len) snprintf(first, first_len, "%s", g_tally.first.c_str());
    g_tally.checked = g_tally.damaged = 0;
    g_tally.first.clear();
}

}  // namespace smo
