// SMO_POISON_LDS (tests): the LDS sibling of SMO_POISON.  No result may depend on what the LDS held when a kernel was launched; LDS is not
// cleared between dispatches, so a padding row, the tail of a ragged tile or a slot of a run-time plan that is read but never written meets
// what the previous workgroup on that CU left — in a test process a finite leftover of the same solve.  With the knob set every launch of
// the library (the hook of smo_common.hpp) is preceded on its stream by lds_fill_kernel, after which every byte of every CU's LDS holds the
// knob's byte.  Here: the one reader of the knob, the fill, the two counters, and the probe behind smo_lds_probe (include/smo.h), which is
// what shows that the fill reaches what a kernel sees.
//
// The fill: workgroups that each claim the device's whole per-workgroup LDS (163 840 bytes on gfx950), so that a CU holds exactly one of
// them; FILL_ROUNDS workgroups per CU; each stores its LDS and then stays for a fixed short time (two s_sleep, about 7 us), many times what
// the dispatcher needs to start the whole grid, so that the first round of workgroups finds every CU free of its siblings and occupies them
// all at once.  No workgroup waits for another: no counter, no barrier across the grid.  Not reached: a CU that work of ANOTHER stream
// holds for the whole fill ("Not seen").
#include <mutex>

#include "smo_common.hpp"

namespace smo {

std::atomic<int> g_lds_poison{-1};

namespace {

constexpr int FILL_THREADS = 1024, FILL_ROUNDS = 2, PROBE_THREADS = 256, MAX_DEVICES = 64;

__global__ __launch_bounds__(FILL_THREADS) void lds_fill_kernel(unsigned long long word, unsigned n16) {
    extern __shared__ ulonglong2 lds_fill_buf[];                     // (indexed as it is: a pointer copy would make the stores flat ones)
    for (unsigned i = threadIdx.x; i < n16; i += FILL_THREADS) lds_fill_buf[i] = make_ulonglong2(word, word);
    __syncthreads();                                                 // every store has landed before the workgroup starts to idle
    __builtin_amdgcn_s_sleep(127);
    __builtin_amdgcn_s_sleep(127);
}

// reads, never writes, the n8 words of this workgroup's own LDS; res[0] += the words that equal `word` (an integer atomic, from lanes that
// found any)
__global__ __launch_bounds__(PROBE_THREADS) void lds_probe_kernel(unsigned long long word, unsigned n8, unsigned long long* res) {
    extern __shared__ unsigned long long lds_probe_buf[];
    unsigned eq = 0;
    for (unsigned i = threadIdx.x; i < n8; i += PROBE_THREADS) eq += lds_probe_buf[i] == word ? 1u : 0u;
    if (eq) atomicAdd(res, (unsigned long long)eq);
}

struct DeviceLds {
    std::atomic<int> ready{0};
    int cus = 0, lds_bytes = 0;
} g_dev[MAX_DEVICES];
std::mutex g_mu;
std::atomic<unsigned long long> g_fills{0}, g_launches{0};

// the current device's LDS per workgroup and CU count; both kernels may then claim all of it (once per device)
int ready_device(int dev) {
    if (dev < 0 || dev >= MAX_DEVICES) { set_error("SMO_POISON_LDS: device %d (at most %d devices)", dev, MAX_DEVICES); return SMO_ERR_ARG; }
    if (g_dev[dev].ready.load(std::memory_order_acquire)) return SMO_OK;
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_dev[dev].ready.load(std::memory_order_relaxed)) return SMO_OK;
    int maxb = 0, cus = 0;
    SMO_HIP(hipDeviceGetAttribute(&maxb, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    SMO_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (maxb < 16 || cus < 1) { set_error("SMO_POISON_LDS: device %d reports %d bytes of LDS and %d CUs", dev, maxb, cus); return SMO_ERR_HIP; }
    SMO_HIP(hipFuncSetAttribute((const void*)lds_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, maxb));
    SMO_HIP(hipFuncSetAttribute((const void*)lds_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, maxb));
    g_dev[dev].cus = cus;
    g_dev[dev].lds_bytes = maxb / 16 * 16;
    g_dev[dev].ready.store(1, std::memory_order_release);
    return SMO_OK;
}

}  // namespace

int lds_poison_read() {
    const char* e = getenv("SMO_POISON_LDS");
    if (!e) { g_lds_poison.store(-1, std::memory_order_relaxed); return SMO_OK; }
    int v = -1;
    if (!lds::parse_byte(e, &v)) {
        set_error("SMO_POISON_LDS must be a whole number in 0..255, got \"%s\"", e);
        return SMO_ERR_ARG;
    }
    int dev = 0;
    SMO_HIP(hipGetDevice(&dev));
    SMO_TRY(ready_device(dev));
    g_lds_poison.store(v, std::memory_order_relaxed);
    return SMO_OK;
}

// Returns nothing: a launch site has no error path of its own ahead of its kernel.  If the device cannot be asked or readied, or the fill
// cannot be launched, the kernel that follows runs unfilled and fills < launches is the error channel — every test of the suite demands
// fills == launches.  A device that no reader of the knob has readied is readied here, which inside a stream capture means a
// hipFuncSetAttribute during the capture; contexts ready their device in base_init, before anything is captured.
void lds_fill(hipStream_t s) {
    g_launches.fetch_add(1, std::memory_order_relaxed);
    const int byte = g_lds_poison.load(std::memory_order_relaxed);
    int dev = 0;
    if (byte < 0 || hipGetDevice(&dev) != hipSuccess || ready_device(dev) != SMO_OK) return;      // (a device no reader has seen: readied here)
    const DeviceLds& d = g_dev[dev];
    SMO_LAUNCH_THE_FILL(lds_fill_kernel, dim3((unsigned)(FILL_ROUNDS * d.cus)), dim3(FILL_THREADS), (size_t)d.lds_bytes, s, lds::fill_word(byte),
                        (unsigned)(d.lds_bytes / 16));
    if (hipPeekAtLastError() == hipSuccess) g_fills.fetch_add(1, std::memory_order_relaxed);
}

void lds_take(size_t* fills, size_t* launches) {
    const unsigned long long f = g_fills.exchange(0, std::memory_order_relaxed), l = g_launches.exchange(0, std::memory_order_relaxed);
    if (fills) *fills = (size_t)f;
    if (launches) *launches = (size_t)l;
}

}  // namespace smo

using namespace smo;

extern "C" int smo_lds_probe(int device, size_t lds_bytes, size_t workgroups, size_t* words, size_t* words_equal_fill, size_t* fills_launched,
                             size_t* launches_hooked) {
    if (words) *words = 0;
    if (words_equal_fill) *words_equal_fill = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { set_error("no usable HIP device; libsmo has no CPU fallback"); return SMO_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (have %d)", device, ndev); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(device));
    SMO_TRY(lds_poison_read());
    if (lds_bytes != 0 && workgroups != 0) {
        SMO_TRY(ready_device(device));
        if (lds_bytes % 8 != 0 || lds_bytes > (size_t)g_dev[device].lds_bytes || workgroups > 65536) {
            set_error("smo_lds_probe: lds_bytes = %zu (a multiple of 8, at most %d), workgroups = %zu (at most 65536)", lds_bytes, g_dev[device].lds_bytes, workgroups);
            return SMO_ERR_ARG;
        }
        const int byte = g_lds_poison.load(std::memory_order_relaxed);
        unsigned long long* res = nullptr;
        unsigned long long h = 0;
        SMO_HIP(hipMalloc(&res, sizeof(h)));
        hipError_t e = hipMemcpy(res, &h, sizeof(h), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            SMO_LAUNCH(lds_probe_kernel, dim3((unsigned)workgroups), dim3(PROBE_THREADS), lds_bytes, nullptr, lds::fill_word(byte < 0 ? 0 : byte),
                       (unsigned)(lds_bytes / 8), res);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpy(&h, res, sizeof(h), hipMemcpyDeviceToHost);
        (void)hipFree(res);
        if (e != hipSuccess) { set_error("smo_lds_probe: %s", hipGetErrorString(e)); return SMO_ERR_HIP; }
        if (words) *words = workgroups * (lds_bytes / 8);
        if (words_equal_fill) *words_equal_fill = (size_t)h;
    }
    lds_take(fills_launched, launches_hooked);
    return SMO_OK;
}
