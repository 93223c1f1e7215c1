// mirhi_api.hip -- implementation of the C ABI declared in include/mirhi.h.
//
// Host-only logic: object lifetimes, validation with the reference's error behaviour
// (crates/rhi/src/{buffer,pipeline,command,sync}.rs), translation of a recorded command buffer
// into kernel launches on a HIP stream (crates/renderer/src/renderer.rs:452-557,
// frame_manager.rs:299-539).  No rasterization arithmetic lives here and there is no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <hsa/amd_hsa_signal.h>
#include <rccl/rccl.h>     // types and prototypes only: librccl is loaded with dlopen on first use (no link-time dependency)

#include "../../include/mirhi.h"
#include "mirhi_device.h"
#include "mirhi_launch.h"
#include "mirhi_variant.h"
#include "mirhi_scope.h"
#include "mirhi_submit.h"

using namespace mirhi;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static mirhi_result fail(mirhi_result code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
static mirhi_result hip_fail(hipError_t e, const char* what) {
    const mirhi_result code = (e == hipErrorOutOfMemory) ? MIRHI_ERR_ALLOCATOR : MIRHI_ERR_DEVICE;
    return fail(code, "%s: %s (%s)", code == MIRHI_ERR_ALLOCATOR ? "Allocator error" : "Vulkan error", hipGetErrorString(e), what);
}
#define HIP_TRY(expr)                                              \
    do {                                                           \
        hipError_t e__ = (expr);                                   \
        if (e__ != hipSuccess) return hip_fail(e__, #expr);        \
    } while (0)
#define NULL_CHECK(p, name)                                        \
    do {                                                           \
        if (!(p)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s is null", name); \
    } while (0)

extern "C" const char* mirhi_last_error_message(void) { return g_last_error.c_str(); }
extern "C" uint32_t mirhi_abi_version(void) { return MIRHI_ABI_VERSION; }
extern "C" const char* mirhi_result_name(mirhi_result r) {
    switch (r) {
        case MIRHI_OK: return "Ok";
        case MIRHI_ERR_DEVICE: return "VulkanError";
        case MIRHI_ERR_LOADING: return "LoadingError";
        case MIRHI_ERR_ALLOCATOR: return "AllocatorError";
        case MIRHI_ERR_NO_SUITABLE_GPU: return "NoSuitableGpu";
        case MIRHI_ERR_SHADER: return "ShaderError";
        case MIRHI_ERR_SURFACE: return "SurfaceError";
        case MIRHI_ERR_SWAPCHAIN: return "SwapchainError";
        case MIRHI_ERR_INVALID_HANDLE: return "InvalidHandle";
        case MIRHI_ERR_PIPELINE: return "PipelineError";
        case MIRHI_ERR_LOCK_POISONED: return "LockPoisoned";
        case MIRHI_TIMEOUT: return "Timeout";
        case MIRHI_NOT_READY: return "NotReady";
        default: return "Unknown";
    }
}

static inline void cpu_relax() { __builtin_ia32_pause(); }

// ------------------------------------------------------------------------------------------------
// native dispatch: AQL packets written by this library (mirhi_native.h)
// ------------------------------------------------------------------------------------------------
#ifndef MIRHI_SOURCE_HASH
#define MIRHI_SOURCE_HASH "unknown"           // build.py passes the hash of csrc/ + include/mirhi.h to BOTH translation units
#endif
extern "C" const char* mirhi_build_id(void) { return MIRHI_SOURCE_HASH; }

namespace mirhi {
struct NativeKernel { uint64_t object; uint32_t kernarg_bytes, lds_bytes, scratch_bytes; };
struct NativeDevice {
    hsa_agent_t agent{};
    hsa_executable_t exe{};
    std::mutex mu;
    std::vector<std::pair<const void*, NativeKernel>> kernels;      // by host function address (a handful: linear search)
    bool ok = false;
    std::string why;
    std::atomic<uint64_t> dispatches{0};
    std::atomic<bool> lost{false};           // a wait on one of this device's queues ran into its deadline: nothing more is dispatched, every wait fails
    std::string lost_why;
    uint64_t timeout_ns = 10000000000ull;    // deadline of every native wait WITHOUT progress (MIRHI_NATIVE_TIMEOUT_MS)
};
struct NativeQueue {
    NativeDevice* nd = nullptr;
    hsa_queue_t* q = nullptr;
    uint8_t* ring = nullptr;                 // kernel arguments: fine-grained device memory, host-written
    size_t ring_bytes = 0;
    uint64_t widx = 0, drained = 0;          // packets written so far / packets known to have completed
    hsa_signal_t drain_sig{};
    uint64_t seen_foreign = 0;               // mirhi_device::foreign_writes at this queue's last system-scope acquire
    bool proxy = false;                      // hsa_queue_create handed out a software queue (a tool intercepts the packets): see native_queue_open
    std::mutex mu;                           // one producer at a time (a host thread that waits for the queue also writes a packet)
};
}  // namespace mirhi
namespace {
// code object v5 implicit kernel arguments as far as the kernels need them (blockIdx / gridDim / blockDim)
struct ImplicitArgs { uint32_t block_count[3]; uint16_t group_size[3]; uint16_t remainder[3]; uint8_t reserved[16]; uint64_t global_offset[3]; uint16_t grid_dims; uint8_t pad[6]; };
static_assert(sizeof(ImplicitArgs) == 72, "implicit argument block (the part this library fills)");
constexpr size_t NATIVE_RING_BYTES = 256 * 1024;
constexpr size_t NATIVE_KERNARG_SLOT = 1024;      // bytes of kernel arguments (explicit + implicit) a packet may have
constexpr uint32_t NATIVE_QUEUE_PACKETS = 1024;

// environment switches read ONCE (getenv walks the whole environment: ~0.1 us each, and a submit asked five of them)
struct NativeEnv {
    int dispatch = 1;            // MIRHI_NATIVE_DISPATCH: 0 off, 1 on where available, 2 required (a device that cannot start it fails to create)
    int system_scope = 0;        // MIRHI_NATIVE_SYSTEM_SCOPE: 1 system scope on every packet, 2 on every scope's first (A/B runs)
    int geom_tpw = 0;            // MIRHI_GEOM_TPW: triangles per geometry wave of small scopes (16 / 32 / 64; 0 = the host's choice)
    bool no_batch = false, fence_record = false;
    uint64_t timeout_ns = 10000000000ull;
    NativeEnv() {
        auto num = [](const char* n, int d) { const char* v = getenv(n); return v ? atoi(v) : d; };
        dispatch = num("MIRHI_NATIVE_DISPATCH", 1); system_scope = num("MIRHI_NATIVE_SYSTEM_SCOPE", 0);
        geom_tpw = num("MIRHI_GEOM_TPW", 0);
        no_batch = getenv("MIRHI_NO_BATCH") != nullptr; fence_record = getenv("MIRHI_FENCE_RECORD") != nullptr;
        const int ms = num("MIRHI_NATIVE_TIMEOUT_MS", 10000);
        timeout_ns = (uint64_t)(ms > 0 ? ms : 10000) * 1000000ull;
    }
};
const NativeEnv& native_env() { static const NativeEnv e; return e; }

struct PickAgent { uint32_t domain, bdf; hsa_agent_t found{}; uint32_t matches = 0; };
hsa_status_t native_pick_agent(hsa_agent_t a, void* data) {
    auto* want = static_cast<PickAgent*>(data);      // PCI domain and bus:device.function of the HIP device
    hsa_device_type_t t;
    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) != HSA_STATUS_SUCCESS || t != HSA_DEVICE_TYPE_GPU) return HSA_STATUS_SUCCESS;
    uint32_t bdf = 0, domain = 0;
    if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
    if (hsa_agent_get_info(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &domain) != HSA_STATUS_SUCCESS) domain = 0;
    if ((bdf & 0xFFFFu) == (want->bdf & 0xFFFFu) && domain == want->domain) { if (want->matches++ == 0) want->found = a; }
    return HSA_STATUS_SUCCESS;
}

// the directory this shared library was loaded from (the code object sits beside it)
// <dir>/<library name without .so>_kernels.hsaco: the code object build.py took out of THIS library's object (libmirhi.so -> libmirhi_kernels.hsaco; a
// variant build beside it -- tools/ab_bench.sh -- finds its own)
std::string native_code_object_path() {
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void*>(&native_code_object_path), &info) || !info.dli_fname) return "./libmirhi_kernels.hsaco";
    std::string p = info.dli_fname;
    const size_t dot = p.rfind(".so");
    if (dot != std::string::npos) p.erase(dot);
    return p + "_kernels.hsaco";
}

mirhi::NativeDevice* native_device_open(int ordinal) {
    auto* nd = new mirhi::NativeDevice();
    auto fail_with = [&](const std::string& w) { nd->why = w; return nd; };
    nd->timeout_ns = native_env().timeout_ns;
    if (native_env().dispatch == 0) return fail_with("switched off (MIRHI_NATIVE_DISPATCH=0)");
    if (hsa_init() != HSA_STATUS_SUCCESS) return fail_with("hsa_init failed");
    int bus = 0, devid = 0, domain = 0;
    if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, ordinal) != hipSuccess || hipDeviceGetAttribute(&devid, hipDeviceAttributePciDeviceId, ordinal) != hipSuccess) { (void)hipGetLastError(); return fail_with("no PCI id for the HIP device"); }
    if (hipDeviceGetAttribute(&domain, hipDeviceAttributePciDomainID, ordinal) != hipSuccess) { (void)hipGetLastError(); domain = 0; }
    // the ROCr agent of the HIP ordinal: PCI domain AND bus:device.function (hosts with several PCI domains repeat bus numbers); an ambiguous match is refused
    PickAgent want; want.domain = (uint32_t)domain; want.bdf = (uint32_t)((bus << 8) | (devid << 3));
    (void)hsa_iterate_agents(native_pick_agent, &want);
    if (want.matches == 0) return fail_with("no ROCr agent with the HIP device's PCI address");
    if (want.matches > 1) return fail_with("several ROCr agents share the HIP device's PCI address");
    nd->agent = want.found;
    const std::string path = native_code_object_path();
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return fail_with(path + " is missing (build.py writes it)");
    std::vector<char> blob;
    { char buf[65536]; size_t n; while ((n = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n); }
    fclose(f);
    hsa_code_object_reader_t reader;
    if (hsa_code_object_reader_create_from_memory(blob.data(), blob.size(), &reader) != HSA_STATUS_SUCCESS) return fail_with("code object reader");
    if (hsa_executable_create_alt(HSA_PROFILE_FULL, HSA_DEFAULT_FLOAT_ROUNDING_MODE_DEFAULT, nullptr, &nd->exe) != HSA_STATUS_SUCCESS) return fail_with("executable create");
    if (hsa_executable_load_agent_code_object(nd->exe, nd->agent, reader, nullptr, nullptr) != HSA_STATUS_SUCCESS) return fail_with("code object load (is " + path + " of this build?)");
    if (hsa_executable_freeze(nd->exe, nullptr) != HSA_STATUS_SUCCESS) return fail_with("executable freeze");
    // The code object must be the one this library was built with: a stale pair with another kernel-argument layout would dispatch garbage.  Both
    // translation units carry the build's source hash (build.py: -DMIRHI_SOURCE_HASH); the code object's copy is the device variable mirhi::g_build_id.
    {
        hsa_executable_symbol_t sym; uint64_t addr = 0; char theirs[32] = {0};
        if (hsa_executable_get_symbol_by_name(nd->exe, "_ZN5mirhi10g_build_idE", &nd->agent, &sym) != HSA_STATUS_SUCCESS ||
            hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_VARIABLE_ADDRESS, &addr) != HSA_STATUS_SUCCESS || !addr ||
            hsa_memory_copy(theirs, reinterpret_cast<void*>(addr), 17) != HSA_STATUS_SUCCESS)
            return fail_with(path + " carries no build id (built by another build.py?)");
        theirs[17] = 0;
        if (strcmp(theirs, MIRHI_SOURCE_HASH) != 0) return fail_with(path + " is of build " + theirs + ", this library of build " MIRHI_SOURCE_HASH);
    }
    nd->ok = true;
    return nd;
}

// the sRGB table of this copy of the code object (the HIP runtime's copy has its own: upload_srgb_lut)
bool native_upload_symbol(mirhi::NativeDevice* nd, const char* name, const void* src, size_t bytes) {
    hsa_executable_symbol_t sym;
    if (hsa_executable_get_symbol_by_name(nd->exe, name, &nd->agent, &sym) != HSA_STATUS_SUCCESS) return false;
    uint64_t addr = 0;
    if (hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_VARIABLE_ADDRESS, &addr) != HSA_STATUS_SUCCESS || !addr) return false;
    return hsa_memory_copy(reinterpret_cast<void*>(addr), src, bytes) == HSA_STATUS_SUCCESS;
}

// Is this queue the hardware's, or a software queue a tool put in front of it?  Under rocprofv3 counter collection (and any tool that registers with ROCr's
// queue-intercept API) hsa_queue_create returns a PROXY: its packets are consumed by a handler that runs inside the doorbell signal's store, rewritten
// (completion signals swapped, PM4 packets put around each dispatch) and copied to the real queue.  On a proxy `read_index` means "copied", not
// "consumed by the packet processor", so nothing about completion may be concluded from it.  The public signal ABI (hsa/amd_hsa_signal.h) tells the two apart:
// a hardware queue's doorbell signal is of kind AMD_SIGNAL_KIND_DOORBELL (a mapped doorbell register), a proxy's is an ordinary user signal.
bool native_queue_is_proxy(const hsa_queue_t* q) {
    const amd_signal_t* s = reinterpret_cast<const amd_signal_t*>(q->doorbell_signal.handle);
    return !s || (s->kind != AMD_SIGNAL_KIND_DOORBELL && s->kind != AMD_SIGNAL_KIND_LEGACY_DOORBELL);
}

mirhi::NativeQueue* native_queue_open(mirhi::NativeDevice* nd) {
    auto* nq = new mirhi::NativeQueue();
    nq->nd = nd;
    if (hsa_queue_create(nd->agent, NATIVE_QUEUE_PACKETS, HSA_QUEUE_TYPE_SINGLE, nullptr, nullptr, UINT32_MAX, UINT32_MAX, &nq->q) != HSA_STATUS_SUCCESS) { delete nq; return nullptr; }
    nq->proxy = native_queue_is_proxy(nq->q);
    nq->widx = hsa_queue_load_write_index_relaxed(nq->q);
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, NATIVE_RING_BYTES, hipDeviceMallocFinegrained) != hipSuccess) { (void)hipGetLastError(); (void)hsa_queue_destroy(nq->q); delete nq; return nullptr; }
    nq->ring = static_cast<uint8_t*>(p); nq->ring_bytes = NATIVE_RING_BYTES;
    if (hsa_signal_create(0, 0, nullptr, &nq->drain_sig) != HSA_STATUS_SUCCESS) { (void)hipFree(p); (void)hsa_queue_destroy(nq->q); delete nq; return nullptr; }
    return nq;
}
void native_queue_close(mirhi::NativeQueue* nq) {
    if (!nq) return;
    (void)hsa_signal_destroy(nq->drain_sig);
    (void)hsa_queue_destroy(nq->q);
    (void)hipFree(nq->ring);
    delete nq;
}

void native_mark_lost(mirhi::NativeDevice* nd, const char* where, const mirhi::NativeQueue* nq) {
    if (nd->lost.exchange(true)) return;
    char buf[320];
    if (nq) snprintf(buf, sizeof buf, "%s: no progress within %.1f s (queue write index %llu, read index %llu%s)", where, (double)nd->timeout_ns * 1e-9,
                     (unsigned long long)nq->widx, (unsigned long long)hsa_queue_load_read_index_relaxed(nq->q), nq->proxy ? ", intercepted queue" : "");
    else snprintf(buf, sizeof buf, "%s: no progress within %.1f s", where, (double)nd->timeout_ns * 1e-9);
    nd->lost_why = buf;
    fprintf(stderr, "mirhi: device lost: %s\n", buf);
}

// Waits until a completion signal reads 0.  Returns 0 done, 1 the caller's timeout expired, 2 device lost.  A frame's fence is due within
// microseconds: poll the word in host memory for 200 us, then block in the runtime (interrupt-driven, in slices of at most 10 ms so that a timeout
// is honoured) -- a thread that waits for seconds of GPU work must not keep a core spinning.  NO wait is unbounded: whatever the caller's timeout,
// when `watch`'s read index has not moved for the device's deadline (MIRHI_NATIVE_TIMEOUT_MS, 10 s) the device is marked lost -- a GPU that stopped
// consuming packets, or a tool between this library and the queue that does something else with them, becomes an error, never a hung thread.
int native_signal_wait(hsa_signal_t sig, uint64_t timeout_ns, mirhi::NativeDevice* nd, const mirhi::NativeQueue* watch, const char* where) {
    static const uint64_t ticks_per_s = [] { uint64_t f = 0; return hsa_system_get_info(HSA_SYSTEM_INFO_TIMESTAMP_FREQUENCY, &f) == HSA_STATUS_SUCCESS && f ? f : 100000000ull; }();
    if (nd && nd->lost.load(std::memory_order_acquire)) return hsa_signal_load_scacquire(sig) == 0 ? 0 : 2;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t progress_at = 0, last_ridx = watch ? hsa_queue_load_read_index_relaxed(watch->q) : 0;
    for (uint32_t it = 0;; it++) {
        if (hsa_signal_load_scacquire(sig) == 0) return 0;
        cpu_relax();
        if ((it & 1023u) != 1023u) continue;
        const uint64_t elapsed = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (timeout_ns != UINT64_MAX && elapsed >= timeout_ns) return 1;
        if (watch) { const uint64_t r = hsa_queue_load_read_index_relaxed(watch->q); if (r != last_ridx) { last_ridx = r; progress_at = elapsed; } }
        if (nd && elapsed - progress_at >= nd->timeout_ns) { native_mark_lost(nd, where, watch); return 2; }
        if (elapsed >= 200000ull) {
            uint64_t slice_ns = 10000000ull;
            if (timeout_ns != UINT64_MAX && timeout_ns - elapsed < slice_ns) slice_ns = timeout_ns - elapsed;
            if (nd && nd->timeout_ns - (elapsed - progress_at) < slice_ns) slice_ns = nd->timeout_ns - (elapsed - progress_at);     // (never asleep past the deadline)
            (void)hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_EQ, 0, slice_ns * ticks_per_s / 1000000000ull + 1ull, HSA_WAIT_STATE_BLOCKED);
        }
    }
}

// Room for one more packet.  Kernel arguments: packet w uses slot w % SLOTS of the ring.  Every packet of this queue carries the barrier bit, so once the
// packet processor has CONSUMED packet j + 1 (read index >= j + 2), packet j has finished and its slot is free: at most SLOTS - 2 packets may be outstanding
// when slot w % SLOTS is written again.  On an intercepted queue the read index says "copied by the tool", nothing about the hardware (native_queue_is_proxy):
// there the queue is drained every SLOTS / 2 packets instead.  The wait is bounded: a read index that stands still for the device's deadline = device lost.
bool native_queue_drain_locked(mirhi::NativeQueue* nq);
bool native_reserve(mirhi::NativeQueue* nq) {
    mirhi::NativeDevice* nd = nq->nd;
    constexpr uint64_t SLOTS = NATIVE_RING_BYTES / NATIVE_KERNARG_SLOT;
    static_assert(SLOTS >= 64 && SLOTS <= NATIVE_QUEUE_PACKETS, "kernarg ring");
    if (nd->lost.load(std::memory_order_acquire)) return false;
    if (nq->proxy) { if (nq->widx - nq->drained >= SLOTS / 2) return native_queue_drain_locked(nq); return true; }
    if (nq->widx - hsa_queue_load_read_index_scacquire(nq->q) <= SLOTS - 2) return true;
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t last = hsa_queue_load_read_index_relaxed(nq->q), progress_ns = 0;
    for (uint32_t spins = 1;; spins++) {          // (back-pressure of a full queue: the producer yields)
        const uint64_t r = hsa_queue_load_read_index_scacquire(nq->q);
        if (nq->widx - r <= SLOTS - 2) return true;
        cpu_relax();
        if ((spins & 4095u) != 0u) continue;
        std::this_thread::yield();
        const uint64_t elapsed = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (r != last) { last = r; progress_ns = elapsed; }
        if (elapsed - progress_ns >= nd->timeout_ns) { native_mark_lost(nd, "waiting for room in an AQL queue", nq); return false; }
    }
}
// Publishes the packet at index nq->widx whose body has been written: header (release), write index, doorbell -- the order ROCr documents for a
// single-producer queue (the index was reserved by this one producer: nq->mu).
void native_publish(mirhi::NativeQueue* nq, void* packet, uint16_t header, uint16_t setup) {
    __atomic_store_n(reinterpret_cast<uint32_t*>(packet), (uint32_t)header | ((uint32_t)setup << 16), __ATOMIC_RELEASE);     // (also orders the kernarg stores: x86 stores stay in order)
    const uint64_t idx = nq->widx++;
    hsa_queue_store_write_index_screlease(nq->q, idx + 1);
    __builtin_ia32_sfence();                                     // the write-combined kernarg stores leave the CPU before the doorbell does
    hsa_signal_store_screlease(nq->q->doorbell_signal, (hsa_signal_value_t)idx);
}

// every packet written to the queue so far has completed (a barrier packet with a completion signal, waited for on the host); false: device lost
bool native_queue_drain_locked(mirhi::NativeQueue* nq) {
    if (nq->drained == nq->widx) return !nq->nd->lost.load(std::memory_order_acquire);
    if (nq->nd->lost.load(std::memory_order_acquire)) return false;
    // (ring room: NATIVE_QUEUE_PACKETS is four times the packets native_reserve lets be outstanding)
    hsa_signal_store_relaxed(nq->drain_sig, 1);
    auto* p = reinterpret_cast<hsa_barrier_and_packet_t*>(nq->q->base_address) + (nq->widx & (NATIVE_QUEUE_PACKETS - 1));
    memset(reinterpret_cast<uint8_t*>(p) + 4, 0, sizeof *p - 4);
    p->completion_signal = nq->drain_sig;
    const uint16_t header = (HSA_PACKET_TYPE_BARRIER_AND << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                            (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
    native_publish(nq, p, header, 0);
    if (native_signal_wait(nq->drain_sig, UINT64_MAX, nq->nd, nq, "draining an AQL queue") != 0) return false;
    nq->drained = nq->widx;
    return true;
}
bool native_queue_drain(mirhi::NativeQueue* nq) {
    if (!nq) return true;
    std::lock_guard<std::mutex> qlock(nq->mu);
    return native_queue_drain_locked(nq);
}
}  // namespace

hipError_t mirhi::native_enqueue(NativeQueue* nq, const void* key, dim3 grid, dim3 block, const void* args, size_t args_bytes, uint64_t signal, uint32_t flags) {
    NativeDevice* nd = nq->nd;
    const NativeKernel* k = nullptr;
    {
        std::lock_guard<std::mutex> lock(nd->mu);
        for (auto& e : nd->kernels) if (e.first == key) { k = &e.second; break; }
        if (!k) {
            hsa_executable_symbol_t sym;
            const char* mangled = hipKernelNameRefByPtr(key, nullptr);         // the device-side symbol the HIP runtime registered for this kernel
            if (!mangled) { (void)hipGetLastError(); return hipErrorInvalidDeviceFunction; }
            const std::string name = std::string(mangled) + ".kd";
            NativeKernel nk{};
            if (hsa_executable_get_symbol_by_name(nd->exe, name.c_str(), &nd->agent, &sym) != HSA_STATUS_SUCCESS ||
                hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_OBJECT, &nk.object) != HSA_STATUS_SUCCESS ||
                hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_KERNARG_SEGMENT_SIZE, &nk.kernarg_bytes) != HSA_STATUS_SUCCESS ||
                hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_GROUP_SEGMENT_SIZE, &nk.lds_bytes) != HSA_STATUS_SUCCESS ||
                hsa_executable_symbol_get_info(sym, HSA_EXECUTABLE_SYMBOL_INFO_KERNEL_PRIVATE_SEGMENT_SIZE, &nk.scratch_bytes) != HSA_STATUS_SUCCESS)
                return hipErrorInvalidDeviceFunction;
            if (nk.scratch_bytes != 0) return hipErrorInvalidDeviceFunction;         // (no kernel of this library uses scratch; a queue of ours has none set up)
            nd->kernels.emplace_back(key, nk);
            k = &nd->kernels.back().second;
        }
    }
    std::lock_guard<std::mutex> qlock(nq->mu);
    const size_t explicit_bytes = (args_bytes + 7) & ~(size_t)7;
    const size_t need = (std::max<size_t>(explicit_bytes + sizeof(ImplicitArgs), k->kernarg_bytes) + 63) & ~(size_t)63;
    if (need > NATIVE_KERNARG_SLOT || explicit_bytes + sizeof(ImplicitArgs) > NATIVE_KERNARG_SLOT) return hipErrorInvalidValue;
    if (!native_reserve(nq)) return hipErrorLaunchTimeOut;          // (device lost: reported as such by the caller)
    constexpr uint64_t SLOTS = NATIVE_RING_BYTES / NATIVE_KERNARG_SLOT;
    uint8_t* ka = nq->ring + (nq->widx % SLOTS) * NATIVE_KERNARG_SLOT;
    alignas(16) uint8_t tmp[NATIVE_KERNARG_SLOT];
    memcpy(tmp, args, args_bytes);
    if (explicit_bytes > args_bytes) memset(tmp + args_bytes, 0, explicit_bytes - args_bytes);
    ImplicitArgs im;
    memset(&im, 0, sizeof im);
    im.block_count[0] = grid.x; im.block_count[1] = grid.y; im.block_count[2] = grid.z;
    im.group_size[0] = (uint16_t)block.x; im.group_size[1] = (uint16_t)block.y; im.group_size[2] = (uint16_t)block.z;
    im.grid_dims = grid.z > 1 ? 3 : (grid.y > 1 ? 2 : 1);
    memcpy(tmp + explicit_bytes, &im, sizeof im);
    memcpy(ka, tmp, explicit_bytes + sizeof im);             // write-combined stores over the BAR
    auto* p = reinterpret_cast<hsa_kernel_dispatch_packet_t*>(nq->q->base_address) + (nq->widx & (NATIVE_QUEUE_PACKETS - 1));
    p->workgroup_size_x = (uint16_t)block.x; p->workgroup_size_y = (uint16_t)block.y; p->workgroup_size_z = (uint16_t)block.z;
    p->reserved0 = 0;
    p->grid_size_x = grid.x * block.x; p->grid_size_y = grid.y * block.y; p->grid_size_z = grid.z * block.z;
    p->private_segment_size = 0; p->group_segment_size = k->lds_bytes;
    p->kernel_object = k->object; p->kernarg_address = ka; p->reserved2 = 0;
    p->completion_signal.handle = signal;
    // every kernel waits for the one before it on its queue (barrier bit); its fences are agent scope unless the caller asked for system scope
    // (a system-scope ACQUIRE costs the packet 2.6 us -- tools/microbench/hsa/hsa_dispatch.cpp -- so it is asked for only when something
    // outside this agent wrote memory since the queue's last one; a completion signal asks for a system-scope RELEASE: the host is told)
    const uint16_t acq = (flags & NATIVE_ACQUIRE_SYSTEM) ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
    const uint16_t rel = (flags & NATIVE_RELEASE_SYSTEM) || signal ? HSA_FENCE_SCOPE_SYSTEM : HSA_FENCE_SCOPE_AGENT;
    const uint16_t header = (HSA_PACKET_TYPE_KERNEL_DISPATCH << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                            (uint16_t)(acq << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (uint16_t)(rel << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE);
    nd->dispatches.fetch_add(1, std::memory_order_relaxed);
    native_publish(nq, p, header, 3 << HSA_KERNEL_DISPATCH_PACKET_SETUP_DIMENSIONS);
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------
// objects
// ------------------------------------------------------------------------------------------------
// One timed dispatch: the event pair is attached to the dispatch itself (hipExtLaunchKernelGGL), so elapsed(start, stop) is
// the kernel's begin -> end on the GPU clock and elapsed(stop of A, stop of B) the distance between two kernels' ends.
struct TimedDispatch { hipEvent_t start, stop; uint32_t kernel, lane; };

struct mirhi_device {
    int ordinal = 0;
    hipStream_t stream = nullptr;           // lane 0
    bool owns_stream = false;
    std::vector<hipStream_t> lanes;          // submit streams; lanes[0] == stream
    uint32_t next_lane = 0;
    std::atomic<int> children{0};
    // Bumped whenever something that is not a kernel of this library writes device memory the kernels may read (copy engines, HIP's
    // memsets, RCCL, memory wrapped from outside): the next scope on each AQL queue then opens with a system-scope acquire; all others
    // open with an agent-scope one (tools/microbench/hsa/stale.cpp: no stale word after any such write even without -- kept as the rule)
    std::atomic<uint64_t> foreign_writes{1};
    uint32_t split_rank = 0, split_world = 1;
    uint32_t split_layout = MIRHI_SPLIT_INTERLEAVED;   // mirhi_device_set_tile_split_layout (MIRHI_SPLIT=bands|interleaved sets the default)
    uint32_t profiling = 0;                  // MIRHI_PROFILE_* bits
    std::mutex mu;
    std::vector<TimedDispatch> pending;       // timed dispatches not yet read back
    std::vector<mirhi_dispatch_time> timeline;   // read back: begin / end relative to the first one since the last reset
    hipEvent_t base_stop = nullptr;           // stop event of that first dispatch (kept until the next reset)
    double base_end_ms = 0.0;                 //   its end on the timeline (= its own duration: the timeline starts at its begin)
    std::vector<hipEvent_t> free_events;
    std::vector<mirhi_cmd*> unchecked;        // submitted since the last wait_idle: their status words are read there
    std::vector<mirhi_fence*> fences;         // live fences (guarded by mu): a command buffer that is destroyed or re-recorded
                                              //   while a fence still lists it hands its device status over first
    std::vector<mirhi_cmd*> cmds;             // live command buffers (guarded by mu): lanes that go away are forgotten by all of them
    std::vector<mirhi_image*> images;         // live images (guarded by mu): a recording may outlive an attachment it names
    hipEvent_t order_event = nullptr;         // cross-lane attachment ordering (mirhi_image::last_stream)
    // native dispatch (mirhi_native.h): one AQL queue per queue lane, opened when the lane first carries a native submit
    NativeDevice* native = nullptr;
    std::vector<NativeQueue*> native_lanes;
    std::vector<hipStream_t> aux_streams;     // streams of the device's communicators (band exchange): wait_idle waits for them, an image they wrote last is ordered behind them
    bool native_on_external = false;          // mirhi_device_set_native_dispatch: lane 0 of a device made on the caller's stream dispatches natively too
    mirhi_result deferred = MIRHI_OK;         // status of such a command buffer that no fence listed: reported by wait_idle
    std::string deferred_msg;
    double total_ms[MIRHI_KERNEL_COUNT] = {0, 0, 0, 0};
    uint64_t launches[MIRHI_KERNEL_COUNT] = {0, 0, 0, 0};
    unsigned long long* frag_stats = nullptr; // device: [0] pixels that ran a fragment program, [1] covered fragments (profiling only)
    uint64_t frag_scopes = 0;                 // scopes counted into frag_stats since the last reset
    mirhi_device_stats stats{};
    char name[256] = {0};
    // Submit thread (mirhi_device_set_submit_thread): vkQueueSubmit hands the work to the driver and returns; with the thread on,
    // mirhi_queue_submit validates, queues the job and returns, and this thread makes the HIP launches (2.3 - 3 us each whatever the
    // entry point, tools/microbench/launch_paths.hip: 5 - 7 us per frame that the render thread then spends recording the next frame).
    // Single producer / single consumer ring; the consumer spins while a frame loop feeds it and sleeps after 100 us without work.
    struct SubmitJob { uint32_t n; mirhi_cmd* cmds[MAX_BATCH > 16 ? MAX_BATCH : 16]; mirhi_fence* fence; };
    static constexpr uint64_t SQ_SLOTS = 64;
    std::thread sq_thread;
    bool sq_on = false;
    SubmitJob sq_ring[SQ_SLOTS];
    std::atomic<uint64_t> sq_pushed{0}, sq_done{0};
    std::atomic<bool> sq_stop{false}, sq_sleeping{false};
    std::mutex sq_mu; std::condition_variable sq_cv;
    std::mutex sq_push_mu;                                    // producers: several host threads may submit to one device (the ring has ONE consumer)
};

struct mirhi_buffer {
    mirhi_device* dev;
    mirhi_buffer_usage usage;
    uint64_t size;
    uint8_t* ptr;
    bool owned;
    bool host_direct = false;   // fine-grained device memory the host stores into (uniform buffers): write_data is a memcpy, as in the reference
};

struct mirhi_image {
    mirhi_device* dev;
    uint32_t width, height;
    mirhi_format format;
    uint8_t* ptr;
    bool owned;
    uint32_t levels = 1;      // mip levels stored contiguously behind level 0 (mirhi_image_generate_mips)
    uint32_t max_anisotropy = 1;   // sampler state (mirhi_image_set_max_anisotropy): 1 = trilinear
    mirhi_sampler_desc sampler = {0, 0, 0, 0, 0};      // ... and the rest of it (mirhi_image_set_sampler): all zero = REPEAT / LINEAR / MIP_LINEAR
    // Layered images (mirhi_image_create_array): `layers` tightly packed width x height levels in one allocation; is_array marks the array object itself,
    // which is no 2-D image (attachments and MIRHI_TEXTURE_SHADOW_MAP take a layer view).  A layer view (mirhi_image_create_layer_view) is a non-owning
    // 2-D image of one layer: ptr points into the array, `parent` is the array -- what attachment ordering resolves a view to (for_each_attachment).
    uint32_t layers = 1; bool is_array = false;
    // Cube images (mirhi_image_create_cube): six faces and `levels` mip levels in one allocation, level-major, then face-major, then row-major; width =
    // height = the edge of level 0, layers = 6.  A cube is neither a 2-D image nor an array: only the mirhi_ibl_* passes, upload and read take one.
    bool is_cube = false;
    // mirhi_image_set_cube_seamless: lookups in this cube filter across face edges and corners (include/mirhi.h "The sampler").  Read when a draw is recorded
    // (mirhi_cmd_bind_ibl / _bind_skybox sets, latched per draw like the sampler state of a texture) and by mirhi_ibl_irradiance / _prefilter for the cube they read.
    uint32_t cube_seamless = 0;
    // Multisampled images (mirhi_image_create_multisampled): samples = 4, the transient attachment of a multisampled scope.  It owns no memory
    // (ptr nullptr, owned false) and is nothing but an attachment: whatever would read or write its texels refuses it (refuse_multisampled).
    uint32_t samples = 1;
    mirhi_image* parent = nullptr;
    uint32_t views = 0;            // live layer views of an array (it cannot be destroyed before them)
    // Attachment ordering across queue lanes: the reference submits everything to one queue, so a scope that LOADs (or overwrites)
    // what an earlier submission rendered is behind it by construction; here two command buffers may sit on different lanes.  The
    // stream, command buffer and submission that used this image as an attachment last: a submit on ANOTHER stream waits for it
    // (one event record + stream wait), unless a fence / wait_idle has reported that submission finished -- the frame loop's case.
    hipStream_t last_stream = nullptr; const mirhi_cmd* last_cmd = nullptr; uint64_t last_seq = 0;
    NativeQueue* last_native = nullptr;      // ... or the AQL queue, when that submission was dispatched natively
};

struct mirhi_pipeline {
    mirhi_device* dev;
    mirhi_pipeline_desc desc;
    mirhi_depth_bias bias;       // the factors of depth_bias_enable (0, 0, 0 through mirhi_pipeline_create: the builder's defaults, pipeline.rs:665-667)
};

// What a rendering scope IS, as opposed to what one of its segments holds (RecordedPass): attachments as they resolved, load / store ops, clear values,
// render area, sample count, views, IBL set.  Zero-filled on construction and without padding bytes, all bytes defined: cut_segment carries it into the
// segment that continues the scope with one assignment and same_recording compares it with one memcmp -- a new scope property is one member here.
struct ScopeHeader {
    // what an attachment resolved to when the scope was recorded: two recordings are the same frame shape only if these agree (an image handle may be a
    // new image at an old address).  zero: always 0 (it fills the struct).
    struct Target { const uint8_t* ptr; uint32_t width, height, format, zero; };
    // the IBL set the scope's MODEL_PBR_IBL draws were recorded under (mirhi_cmd_bind_ibl; one per scope, all its segments): resolved like the targets
    struct IblSet {
        const uint8_t *irradiance, *prefiltered, *lut;
        uint32_t irr_size, pre_size, pre_levels, lut_size;
        uint32_t seamless, zero;           // the two cubes' seamless states when the draw was recorded (bit 0 irradiance, bit 1 prefiltered): part of the set's identity
        bool operator==(const IblSet& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    };
    // a multisampled scope (mirhi_cmd_begin_rendering_resolve): the ops and targets name its RESOLVE images; a multiview scope: depth is the ARRAY's base
    // with ONE layer's extent; a depth-only scope: color has the depth image's extent, no address and format UNDEFINED
    Target color, depth, prim;
    IblSet ibl;
    const uint8_t* view_base;              // view v of a multiview scope reads its light matrix at view_base + v * view_stride (the constants buffer's address + view_offset)
    int32_t color_load_op, color_store_op, depth_load_op, depth_store_op;
    float clear_color[4], clear_depth;     // (compared by their bits)
    int32_t area[4];                       // the render area, the full extent spelled out (take_render_area)
    uint32_t depth_only;                   // no colour attachment: SHADOW draws into the depth image (raster_kernel_depth)
    uint32_t samples;                      // 1, or 4: a multisampled scope
    uint32_t view_mask, view_stride, zero; // a multiview depth scope (mirhi_cmd_begin_rendering_multiview): view_mask != 0; depth_only is set
    ScopeHeader() { memset(this, 0, sizeof *this); samples = 1u; }
    bool operator==(const ScopeHeader& o) const { return memcmp(this, &o, sizeof *this) == 0; }
};
static_assert(sizeof(ScopeHeader::Target) == sizeof(void*) + 4 * 4 && sizeof(ScopeHeader::IblSet) == 3 * sizeof(void*) + 6 * 4, "no padding bytes: memcmp compares them");
static_assert(sizeof(ScopeHeader) == 3 * sizeof(ScopeHeader::Target) + sizeof(ScopeHeader::IblSet) + sizeof(void*) + (4 + 5 + 4 + 5) * 4, "no padding bytes: memcmp compares headers");

// One segment of a rendering scope (a scope is cut where its pipelines change the depth state: cut_segment), or one transfer command.
struct RecordedPass {
    ScopeHeader scope;
    // the attachments' handles: what for_each_attachment orders across lanes, no part of what a recording is (a multiview scope's depth: the ARRAY)
    struct Images { mirhi_image* color = nullptr; mirhi_image* depth = nullptr; mirhi_image* prim_id = nullptr; } images;
    DepthState state;                      // depth / blend state of the segment's draws (mirhi_scope.h)
    std::vector<DrawDesc> draws;
    std::vector<uint64_t> draw_vb_bytes;   // bytes of the bound vertex buffer range per draw (vertex pre-pass extent)
    uint32_t total_tris = 0;
    uint32_t first_tri = 0;                // primitive ids continue across the segments of a scope
    bool carry_in = false, carry_out = false;      // depth is carried through the depth attachment or, without one, a transient buffer of the workspace
    std::vector<mirhi_image*> sampled;     // shadow maps the scope's draws sample (MIRHI_TEXTURE_SHADOW_MAP): ordered like attachments
    // A SKYBOX segment: the one SKYBOX draw it consists of, as PassParams takes it (the sky_ words), fixed when the draw was recorded -- push
    // constants, viewport, scissor and the environment are latched per draw.  All bytes defined (memcmp compares two recordings).
    struct SkyDraw {
        uint32_t on, visible, size, levels;
        const uint8_t* env;
        int32_t a[3], b[3], scissor[4];
        long long e0[3];
        float pos0[3], posx[3], posy[3];
        uint32_t depth_bits, compare, write, prim;
        uint32_t seamless;                 // the environment's seamless state when the draw was recorded
        SkyDraw() { memset(this, 0, sizeof *this); }
        bool operator==(const SkyDraw& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    } sky;
    // A recorded transfer command (mirhi_cmd_copy_* / _blit_image / _clear_*): an entry of its own with no attachments, draws, bins or vertex job.
    // kind: XFER_* (XFER_NONE: the entry is a rendering scope); the regions as the kernels take them, resolved when the command was recorded; the images
    // are in `sampled` (ordered across lanes like attachments); span: [0, 1) the source buffer's bytes, [2, 3) the destination buffer's (recording_reads).
    // All bytes defined (memcmp compares two recordings).
    struct Transfer {
        uint32_t kind, count, src_format, dst_format;
        float color[4];
        uint32_t groups, grid;      // work units of all regions; workgroups of the launch
        const uint8_t* span[4];
        Transfer() { memset(this, 0, sizeof *this); }
        bool operator==(const Transfer& o) const { return memcmp(this, &o, sizeof *this) == 0; }
    } xfer;
    std::vector<XferRegion> xfer_regions;
};

// Words of the counter block that never move (a re-recorded frame of another shape finds them where the last frame's kernels
// left them, re-armed): the two big-list counters, the eight pool counters a cache line apart; the bin counters follow.
constexpr uint32_t CTR_BIG = 0u, CTR_POOL = 32u, CTR_ACTIVE = CTR_POOL + 8u * (uint32_t)POOL_COUNTER_STRIDE,   // busy-tile counters: two parities x 8 x 32 words
                   CTR_BINS = CTR_ACTIVE + 2u * 8u * 32u + 32u;

// A bin set: the five device buffers a rendering scope works against -- bin pool, page table, counter block, big-triangle list, vertex output -- as
// `slots` equal slices, one hipMalloc per buffer.  A command buffer has two (Workspace): the scopes' own, of one slot, and the view slots' of its multiview
// scopes, of up to MAX_BATCH, so that the views of a scope run side by side and leave the scopes' set alone.  The slices only grow, and the kernels
// leave counters and tables re-armed; a slot's big-list parity flips when the slot is used, whatever the other slots and the other set do.
struct BinSet {
    BinRec* pool = nullptr; size_t pool_bytes = 0;              // pages of BIN_PAGE_RECS records: fixed first pages, then the dynamic ones
    uint32_t* table = nullptr; size_t table_bytes = 0;          // [tiles][BIN_TABLE_ROW] page table, PAGE_EMPTY when idle
    uint32_t* counters = nullptr; size_t counters_bytes = 0;    // CTR_*: two big-list counters, the pool counters, the busy-tile counters, the bin counts
    BigRec* big = nullptr; size_t big_bytes = 0;
    uint8_t* vs = nullptr; size_t vs_bytes = 0;
    struct Strides { size_t pages = 0, tiles = 0, counter_words = 0, big_cap = 0, vs_bytes = 0; } stride;      // of one slot, in the units named
    uint32_t slots = 0;
    uint32_t parity = 0;                                        // bit j: which of slot j's two big-list counters its next scope appends to
    bool dirty = true;                                          // counters / page table not known to be in their idle state: cleared at the next plan
    // slot j's base pointers (and the pages of its pool): all that anything downstream of the growth knows of the slices
    struct Slot { BinRec* pool; size_t pages; uint32_t* table; uint32_t* counters; BigRec* big; uint8_t* vs; };
    Slot slot(size_t j) const {
        return Slot{pool + j * stride.pages * BIN_PAGE_RECS, stride.pages, table + j * stride.tiles * BIN_TABLE_ROW, counters + j * stride.counter_words, big + j * stride.big_cap,
                    vs + j * stride.vs_bytes};
    }
    uint32_t parity_of(uint32_t j) const { return (parity >> j) & 1u; }
    uint32_t take_parity(uint32_t j) { const uint32_t p = parity_of(j); parity ^= 1u << j; return p; }      // the slot's current parity; its next scope gets the other
    size_t bytes() const { return pool_bytes + table_bytes + counters_bytes + big_bytes + vs_bytes; }
    void free_buffers() { for (void* p : {(void*)pool, (void*)table, (void*)counters, (void*)big, (void*)vs}) if (p) (void)hipFree(p); }
};

// Where the pieces of the parameter block start (bytes, each 256-aligned): [2 x PassParams per scope][draw descriptors][transfer regions][vertex jobs], and
// behind them what the views of multiview scopes read: [2 x PassParams per view slot][their draw descriptors][their vertex jobs].  `bytes`: all of it (without
// a multiview scope the block ends behind the scopes' vertex jobs).
struct BlockLayout {
    size_t draws = 0, regions = 0, jobs = 0, view_params = 0, view_draws = 0, view_jobs = 0, bytes = 0;
    // the device copy of scope `pi` / of view slot `slot` of the plan (mirhi_cmd::ViewSet::first + j) for big-list parity `parity`
    static size_t scope_params(size_t pi, uint32_t parity) { return (2 * pi + parity) * sizeof(PassParams); }
    size_t slot_params(size_t slot, uint32_t parity) const { return view_params + (2 * slot + parity) * sizeof(PassParams); }
};
static BlockLayout block_layout(size_t scopes, size_t draws, size_t regions, size_t jobs, size_t views, size_t view_draws, size_t view_jobs) {
    auto align256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    BlockLayout l;
    l.draws = align256(scopes * 2 * sizeof(PassParams));
    l.regions = align256(l.draws + draws * sizeof(DrawDesc));
    l.jobs = align256(l.regions + regions * sizeof(XferRegion));
    l.bytes = l.jobs + jobs * sizeof(VsJob);
    l.view_params = align256(l.bytes);
    l.view_draws = align256(l.view_params + views * 2 * sizeof(PassParams));
    l.view_jobs = align256(l.view_draws + view_draws * sizeof(DrawDesc));
    if (views) l.bytes = l.view_jobs + view_jobs * sizeof(VsJob);
    return l;
}

struct Workspace {
    // Parameter block: everything the kernels read as "parameters" -- two PassParams per scope (big-list counter parity 0 / 1), the
    // draw descriptors, the vertex pre-pass jobs -- in ONE piece of fine-grained device memory that the host writes directly
    // (stores over the PCIe BAR, 0.2 us per KB; tools/microbench/fence_latency.hip) and only when its bytes changed: re-recording
    // an unchanged frame uploads nothing, a changed one costs a memcpy, and no copy command ever enters a stream.  `pshadow` is the
    // host's copy of what the block holds (device memory is never read back over the BAR).
    uint8_t* pblock = nullptr; size_t pblock_bytes = 0; bool pblock_direct = false;   // direct: host-writable; else uploads go through `pstage`
    bool foreign = false;                                                             // the block went up through a copy engine (fallback): the next scope acquires at system scope
    uint8_t* pstage = nullptr; size_t pstage_bytes = 0;                                // pinned staging for the fallback (hipMemcpyAsync on the lane)
    std::vector<uint8_t> pshadow, pimage;                                              // what the block holds / what it should hold
    BlockLayout layout;                                                                // where its pieces start
    BinSet scope_bins, view_bins;                              // the scopes' bins (one slot) and those of the multiview scopes' view slots
    uint32_t pool_scale = 1;                                   // doubled whenever a scope exhausted the pool (applied at the next submit)
    bool grow_pool = false;
    // Feedback on the two-team mesh mode (raster_mode picks it from the triangle count alone: 'few triangles per tile' is a mesh
    // that sits in a part of the frame -- or one spread thinly over all of it, where the wider workgroups only cost occupancy): a
    // scope that ran in that mode and opened more than two list pages per tile of the frame was spread out (64x64-quad grid over a
    // 1080p frame: 5,340 pages on 2,040 tiles, raster 41.8 us with two teams, 30.4 us with one; the dancer asset: 1,770 pages, 39 us
    // against 66 us); the plan is rebuilt with one team.
    bool spread = false, replan = false;
    // Feedback on the wide mesh variant (sixteen waves per tile: raster_body, WIDE): the busy tiles the scope before last reported.  A mesh
    // scope whose triangles sit in at most WIDE_ON tiles leaves most of the chip without work -- every busy tile then gets four times the
    // waves; above WIDE_OFF it goes back (hysteresis: a frame loop must not flip between two plans).
    uint32_t busy_tiles = 0; bool busy_known = false, wide_eligible = false;
    uint32_t wide = 0;                                         // waves per tile of the wide variant in use: 0 (four waves), 8 or 16
    uint64_t spread_tris = 0;                                  // triangles of the command buffer when `spread` was measured: forgotten when the
                                                               // recorded frame is another one (more than twice / less than half as many)
    uint32_t xcd_tiles_last = 0;                               // tiles of the command buffer's last scope if it uses per-XCD bins, else 0
    float* carry_depth = nullptr; size_t carry_depth_bytes = 0;   // depth hand-over between the segments of a scope without a depth attachment
    TriRec* ordered = nullptr; size_t ordered_bytes = 0;          // slot t = triangle t of an ordered segment (blending)
    PassParams* params = nullptr;                            // = pblock: two copies per scope (big-list counter parity 0 / 1), read by the kernels
    uint32_t* flat_color = nullptr; size_t flat_color_bytes = 0;
    uint32_t* prim_draw = nullptr; size_t prim_draw_bytes = 0;     // per primitive: its draw (scopes with several draws)
    uint32_t* status_host = nullptr;                             // pinned, device-mapped: [status bits, big-list length]
    uint32_t* status_dev = nullptr;                              // device view of status_host
    // re-arms the four words the kernels report in, and the four of each view slot of a multiview scope behind them (STATUS_WORDS in all)
    static constexpr uint32_t STATUS_VIEWS = 16u, STATUS_WORDS = STATUS_VIEWS + 4u * (uint32_t)MAX_BATCH;
    void clear_status() { for (uint32_t i = 0; i < STATUS_WORDS; i++) status_host[i] = 0; }
    // status bits of the last submission: the scopes' own and those of every view slot
    uint32_t status_bits() const { uint32_t b = status_host[0]; for (uint32_t j = 0; j < (uint32_t)MAX_BATCH; j++) b |= status_host[STATUS_VIEWS + 4u * j]; return b; }
    bool any_status() const { uint32_t b = 0; for (uint32_t i = 0; i < STATUS_WORDS; i++) b |= status_host[i]; return b != 0; }
    // statistics pass (MIRHI_PROFILE_FRAGMENTS), built on first use: a primitive-id image of the workspace's own and copies
    // of the scopes' parameters that write it, so that the product kernels and parameters stay untouched
    uint32_t* stats_prim = nullptr; size_t stats_prim_bytes = 0;
    PassParams* stats_params = nullptr; size_t stats_params_bytes = 0; bool stats_params_valid = false;
    // (what bench.py reports and test_gpu_parity bounds: the parameter block, the two bin sets and the flat colours -- carry_depth, ordered, prim_draw and the
    // statistics buffers have never been counted)
    size_t bytes() const { return pblock_bytes + scope_bins.bytes() + view_bins.bytes() + flat_color_bytes; }
};

enum CmdState { CMD_INITIAL = 0, CMD_RECORDING = 1, CMD_EXECUTABLE = 2 };

struct mirhi_cmd {
    mirhi_device* dev;
    CmdState state = CMD_INITIAL;
    uint32_t lane = 0;                     // submit stream of this command buffer (frames in flight overlap across lanes)
    hipStream_t last_stream = nullptr;     // the stream its last submission ran on (a batched submit runs on the first command buffer's lane)
    bool pending = false;                  // submitted and not yet known to have finished (a fence wait / wait_idle clears it).  Vulkan forbids
                                           //   re-recording a pending command buffer; this build synchronises instead -- the slow path a frame
                                           //   loop that waits on its fences never takes
    uint64_t submit_seq = 0;               // submissions so far (a fence remembers which one it saw)
    std::atomic<int> queued{0};            // submissions handed to the submit thread and not yet issued by it
    NativeQueue* last_native = nullptr;    // its last submission went out as AQL packets on this queue (else: last_stream)
    bool one_time = true;
    bool in_rendering = false;
    std::vector<RecordedPass> passes;
    // Plan cache: the recording the current plan was built from.  A frame loop records the same frame again and again
    // (renderer.rs:452-557); end() then finds plan, workspace and parameter block as they are and touches nothing.
    std::vector<RecordedPass> planned;
    bool plan_valid = false;
    uint32_t plan_split_rank = 0, plan_split_world = 1, plan_split_layout = 0;
    // current bindings (dynamic state + descriptors)
    mirhi_pipeline* pipeline = nullptr;
    mirhi_buffer* vb = nullptr; uint64_t vb_offset = 0;
    mirhi_buffer* ib = nullptr; uint64_t ib_offset = 0; mirhi_index_type ib_type = MIRHI_INDEX_UINT32;
    struct { mirhi_buffer* buf; uint64_t offset, range; } uniforms[MIRHI_SLOT_COUNT] = {};
    mirhi_image* textures[MIRHI_TEXTURE_COUNT] = {};
    mirhi_image* cascades = nullptr;       // mirhi_cmd_bind_shadow_cascades: the D32 array (t10) ...
    struct { mirhi_buffer* buf; uint64_t offset, range; } cascade_params = {};      // ... and its CSMParams (b3 of set 2)
    float cascade_blend = 0.0f;            // mirhi_cmd_bind_shadow_cascades_blended: blendThreshold, latched per draw with the binding (0: CalculateShadowCSM)
    mirhi_image* ibl[3] = {};              // mirhi_cmd_bind_ibl: irradiance cube, prefiltered cube, BRDF LUT (set 3); all three or none
    mirhi_image* skybox = nullptr;         // mirhi_cmd_bind_skybox: the environment cube of SKYBOX draws (set 0 of pixel/skybox.hlsl)
    bool has_viewport = false, has_scissor = false;
    uint8_t push_constants[128] = {0};     // vkCmdPushConstants: bytes [0, 64) are a SKYBOX draw's inverseViewProjection, latched when it is recorded
    mirhi_viewport viewport{};
    mirhi_rect2d scissor{};
    // device-side plan, built at end()
    Workspace ws;
    std::vector<PassParams> plan;
    std::vector<uint32_t> plan_programs;
    uint64_t plan_tris = 0;
    // multiview scopes of the plan: per entry of `plan` its view slots (count 0: a single-view scope) and where their parameters start -- `first` counts view
    // slots of the whole plan: plan_view_params[first + j] is slot j's host copy, its two device copies are at BlockLayout::slot_params(first + j, parity)
    struct ViewSet { uint32_t count = 0; size_t first = 0; };
    std::vector<ViewSet> plan_views;
    std::vector<PassParams> plan_view_params;
};

struct mirhi_fence {
    mirhi_device* dev;
    hipEvent_t event = nullptr;
    hipEvent_t join = nullptr;   // cross-lane join for multi-command submits
    bool signaled = false;      // host-visible signaled state
    bool pending = false;       // an event record is outstanding
    std::atomic<bool> issued{true};   // false while its submission waits in the submit thread's queue (the event is recorded when it is issued)
    hsa_signal_t native_sig{0};       // native dispatch: completion signal of the submission's last packet (1 -> 0), polled in host memory
    bool native_wait = false;         //   the pending submission is waited for through it, not through `event`
    NativeQueue* native_q = nullptr;  //   the queue that carries it (its read index is the progress a bounded wait watches)
    std::vector<mirhi_cmd*> cmds;  // submissions to check for device status on completion
    std::vector<uint64_t> seqs;    //   and which submission of each it was (mirhi_cmd::submit_seq)
    mirhi_result deferred = MIRHI_OK;   // status handed over by a listed command buffer that was destroyed / re-recorded since
    std::string deferred_msg;
};

// the command buffer's last submission is known to have finished
static inline void cmd_finished(mirhi_cmd* c) { c->pending = false; }

static uint32_t format_bpp(mirhi_format f) {
    switch (f) {
        case MIRHI_FORMAT_B8G8R8A8_SRGB: case MIRHI_FORMAT_D32_SFLOAT: case MIRHI_FORMAT_R8G8B8A8_UNORM:
        case MIRHI_FORMAT_R8G8B8A8_SRGB: case MIRHI_FORMAT_R32_UINT: return 4;
        case MIRHI_FORMAT_R32G32B32A32_SFLOAT: return 16;
        default: return 0;
    }
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
extern "C" mirhi_result mirhi_device_count(int32_t* out_count) {
    NULL_CHECK(out_count, "out_count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out_count = 0; (void)hipGetLastError(); return MIRHI_OK; }
    *out_count = n;
    return MIRHI_OK;
}

static mirhi_result device_create_common(int32_t ordinal, void* stream, bool external, mirhi_device** out) {
    NULL_CHECK(out, "out");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(MIRHI_ERR_NO_SUITABLE_GPU, "No suitable GPU found"); }
    if (ordinal < 0 || ordinal >= n) return fail(MIRHI_ERR_NO_SUITABLE_GPU, "No suitable GPU found (ordinal %d of %d)", ordinal, n);
    HIP_TRY(hipSetDevice(ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ordinal));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MIRHI_ERR_NO_SUITABLE_GPU, "No suitable GPU found (device %d is %s, kernels are built for gfx950)", ordinal, prop.gcnArchName);
    mirhi_device* d = new (std::nothrow) mirhi_device();
    if (!d) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    d->ordinal = ordinal;
    if (const char* sp = getenv("MIRHI_SPLIT")) d->split_layout = strcmp(sp, "bands") == 0 ? (uint32_t)MIRHI_SPLIT_BANDS : (uint32_t)MIRHI_SPLIT_INTERLEAVED;
    snprintf(d->name, sizeof d->name, "%s (%s)", prop.name, prop.gcnArchName);
    if (external) { d->stream = (hipStream_t)stream; d->owns_stream = false; }
    else {
        hipError_t se = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
        if (se != hipSuccess) { delete d; return hip_fail(se, "hipStreamCreateWithFlags"); }
        d->owns_stream = true;
    }
    d->lanes.push_back(d->stream);
    {
        const hipError_t fe = hipMalloc((void**)&d->frag_stats, 2 * sizeof(unsigned long long));
        // (nothing here goes through the NULL stream: it would claim one of the process's few hardware queues -- ROCclr keeps
        // GPU_MAX_HW_QUEUES = 4 and lets further streams share them -- and two queue lanes that share a hardware queue run their
        // frames one after the other: C2 12.7 us per frame instead of 8.0, tools/saturation_probe.py)
        if (fe != hipSuccess || hipMemsetAsync(d->frag_stats, 0, 2 * sizeof(unsigned long long), d->stream) != hipSuccess) {
            if (d->owns_stream) (void)hipStreamDestroy(d->stream);
            delete d; (void)hipGetLastError();
            return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc for the device statistics block");
        }
    }
    {   // sRGB EOTF per byte, evaluated in double and rounded once (the oracle builds the identical table)
        float lut[256];
        for (int i = 0; i < 256; i++) {
            const double c = (double)i / 255.0;
            lut[i] = (float)(c <= 0.04045 ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4));
        }
        hipError_t le = upload_srgb_lut(lut, d->stream);
        if (le == hipSuccess) le = hipStreamSynchronize(d->stream);
        if (le != hipSuccess) { if (d->owns_stream) (void)hipStreamDestroy(d->stream); delete d; return hip_fail(le, "sRGB table upload"); }
        // native dispatch: the same kernels through our own AQL queues (mirhi_native.h); its copy of the code object has its own table
        d->native = native_device_open(ordinal);
        if (d->native->ok && !native_upload_symbol(d->native, "_ZN5mirhi10g_srgb_lutE", lut, sizeof lut)) { d->native->ok = false; d->native->why = "sRGB table symbol not found in the code object"; }
        d->native_lanes.assign(1, nullptr);
        if (!d->native->ok && native_env().dispatch == 2) {      // (2: required -- tests that must not pass on the fallback)
            const std::string why = d->native->why;
            if (d->owns_stream) (void)hipStreamDestroy(d->stream);
            delete d->native; delete d;
            return fail(MIRHI_ERR_LOADING, "Loading error: native dispatch unavailable: %s", why.c_str());
        }
    }
    *out = d;
    if (getenv("MIRHI_SUBMIT_THREAD") && atoi(getenv("MIRHI_SUBMIT_THREAD")) != 0) (void)mirhi_device_set_submit_thread(d, 1);   // (test runs: every device with the thread on)
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_create(int32_t ordinal, mirhi_device** out) { return device_create_common(ordinal, nullptr, false, out); }
extern "C" mirhi_result mirhi_device_create_on_stream(int32_t ordinal, void* stream, mirhi_device** out) { return device_create_common(ordinal, stream, true, out); }

// every job handed to the submit thread has been issued to the GPU's queues (not: has finished)
static void drain_submits(mirhi_device* dev) {
    if (!dev->sq_on) return;
    const uint64_t want = dev->sq_pushed.load(std::memory_order_acquire);
    while (dev->sq_done.load(std::memory_order_acquire) < want) cpu_relax();
}

// A native wait ran into its deadline (native_mark_lost): the device is gone as far as this library can tell -- VK_ERROR_DEVICE_LOST
static mirhi_result device_lost(mirhi_device* dev) {
    return fail(MIRHI_ERR_DEVICE, "Vulkan error: DEVICE_LOST: %s", dev->native ? dev->native->lost_why.c_str() : "native dispatch");
}
static bool drain_native(mirhi_device* dev, const NativeQueue* which) {      // drains `which` if it is (still) one of the device's queues; false: device lost
    for (NativeQueue* q : dev->native_lanes) if (q && q == which) return native_queue_drain(q);
    return true;
}
static mirhi_result sync_all_lanes(mirhi_device* dev) {
    drain_submits(dev);
    HIP_TRY(hipSetDevice(dev->ordinal));
    bool ok = true;
    for (NativeQueue* nq : dev->native_lanes) ok = native_queue_drain(nq) && ok;
    for (hipStream_t st : dev->lanes) HIP_TRY(hipStreamSynchronize(st));
    for (hipStream_t st : dev->aux_streams) HIP_TRY(hipStreamSynchronize(st));
    return ok ? MIRHI_OK : device_lost(dev);
}
// the AQL queue of a queue lane (opened on first use; native_lanes is sized with the lanes -- mirhi_device_set_queue_lanes -- so that threads that walk it
// never see it move); nullptr: native dispatch is not available
static NativeQueue* native_lane(mirhi_device* dev, uint32_t lane) {
    if (!dev->native || !dev->native->ok || dev->native->lost.load(std::memory_order_acquire) || lane >= dev->native_lanes.size()) return nullptr;
    if (!dev->native_lanes[lane]) {
        NativeQueue* nq = native_queue_open(dev->native);
        if (!nq) { dev->native->ok = false; dev->native->why = "could not open an AQL queue"; return nullptr; }
        if (nq->proxy && native_env().dispatch != 2) {
            // A tool sits between this library and the hardware queue (rocprofv3 --pmc, anything on ROCr's queue-intercept API): its packets would be
            // rewritten and the read index would stop meaning what the producer relies on.  The launches go through HIP, whose queues the tool expects.
            native_queue_close(nq);
            dev->native->ok = false; dev->native->why = "the AQL queue is intercepted by a tool (software doorbell): launches go through HIP";
            return nullptr;
        }
        dev->native_lanes[lane] = nq;
    }
    return dev->native_lanes[lane];
}
static mirhi_result check_status_words(mirhi_device* dev);
extern "C" mirhi_result mirhi_device_set_submit_thread(mirhi_device* dev, uint32_t enable);
extern "C" mirhi_result mirhi_device_wait_idle(mirhi_device* dev) {
    NULL_CHECK(dev, "device");
    mirhi_result r = sync_all_lanes(dev);
    if (r != MIRHI_OK) return r;
    return check_status_words(dev);         // a frame that went wrong on the device fails here too, not only at a fence
}
extern "C" mirhi_result mirhi_device_set_queue_lanes(mirhi_device* dev, uint32_t lanes) {
    NULL_CHECK(dev, "device");
    if (lanes < 1 || lanes > 8) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: queue lanes must be 1..8 (got %u)", lanes);
    mirhi_result r = sync_all_lanes(dev);
    if (r != MIRHI_OK) return r;
    if (dev->lanes.size() > lanes) {
        // (a command buffer must not keep the handle of a stream that is about to go: ADVICE r2, mirhi_cmd::last_stream)
        std::lock_guard<std::mutex> lock(dev->mu);
        for (mirhi_cmd* c : dev->cmds) { c->last_stream = nullptr; c->last_native = nullptr; cmd_finished(c); }
        for (mirhi_image* img : dev->images) { img->last_stream = nullptr; img->last_native = nullptr; img->last_cmd = nullptr; }
    }
    while (dev->lanes.size() > lanes) { (void)hipStreamDestroy(dev->lanes.back()); dev->lanes.pop_back(); }
    {
        std::lock_guard<std::mutex> lock(dev->mu);
        while (dev->native_lanes.size() > lanes) { native_queue_close(dev->native_lanes.back()); dev->native_lanes.pop_back(); }
        dev->native_lanes.resize(lanes, nullptr);
    }
    while (dev->lanes.size() < lanes) {
        hipStream_t st = nullptr;
        HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        dev->lanes.push_back(st);
    }
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_destroy(mirhi_device* dev) {
    NULL_CHECK(dev, "device");
    if (dev->children.load() != 0)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: device still has %d live child objects", dev->children.load());
    (void)mirhi_device_set_submit_thread(dev, 0);
    (void)sync_all_lanes(dev);
    for (size_t i = 1; i < dev->lanes.size(); i++) (void)hipStreamDestroy(dev->lanes[i]);
    for (auto& p : dev->pending) { if (p.start != dev->base_stop) (void)hipEventDestroy(p.start); if (p.stop != dev->base_stop) (void)hipEventDestroy(p.stop); }
    if (dev->base_stop) (void)hipEventDestroy(dev->base_stop);
    for (auto& e : dev->free_events) (void)hipEventDestroy(e);
    if (dev->frag_stats) (void)hipFree(dev->frag_stats);
    if (dev->order_event) (void)hipEventDestroy(dev->order_event);
    for (NativeQueue* nq : dev->native_lanes) native_queue_close(nq);
    if (dev->native) {
        if (dev->native->exe.handle) (void)hsa_executable_destroy(dev->native->exe);
        delete dev->native;
    }
    if (dev->owns_stream) (void)hipStreamDestroy(dev->stream);
    delete dev;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_name(mirhi_device* dev, char* out, uint32_t out_len) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    if (out_len == 0) return MIRHI_OK;
    snprintf(out, out_len, "%s", dev->name);
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_set_tile_split(mirhi_device* dev, uint32_t rank, uint32_t world) {
    NULL_CHECK(dev, "device");
    if (world == 0 || rank >= world) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: tile split rank %u of %u", rank, world);
    drain_submits(dev);
    dev->split_rank = rank; dev->split_world = world;
    return MIRHI_OK;
}
// The tile rows of a frame of `tiles_y` rows that `rank` of `world` rasterizes: rows first + k * step, k < count (PassParams::tile_row_*).
//   bands        one contiguous band per rank, ceil(tiles_y / world) rows, the last rank short: step 1
//   interleaved  rank r owns rows r, r + world, r + 2 world, ...: every rank gets the same share of every part of the frame, whatever the scene puts where
//                (SURVEY 8e's load-balance option; C5 in eight bands: 71 | 72 | 70 | 66 | 53 | 24 | 11 | 5 us of raster -- the slowest rank sets the frame)
static void split_rows(uint32_t layout, uint32_t rank, uint32_t world, uint32_t tiles_y, uint32_t* first, uint32_t* step, uint32_t* count) {
    if (world <= 1) { *first = 0; *step = 1; *count = tiles_y; return; }
    if (layout == MIRHI_SPLIT_BANDS) {
        const uint32_t per = (tiles_y + world - 1) / world;
        uint32_t b = rank * per, e = b + per;
        if (b > tiles_y) b = tiles_y;
        if (e > tiles_y) e = tiles_y;
        *first = b; *step = 1; *count = e - b;
        return;
    }
    *first = rank; *step = world; *count = rank < tiles_y ? (tiles_y - rank + world - 1) / world : 0u;
}
extern "C" mirhi_result mirhi_device_set_tile_split_layout(mirhi_device* dev, mirhi_split_layout layout) {
    NULL_CHECK(dev, "device");
    if (layout != MIRHI_SPLIT_BANDS && layout != MIRHI_SPLIT_INTERLEAVED) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown tile split layout %d", (int)layout);
    drain_submits(dev);
    dev->split_layout = (uint32_t)layout;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_split_rows(mirhi_device* dev, uint32_t height, uint32_t* first_tile_row, uint32_t* tile_row_step, uint32_t* tile_rows) {
    NULL_CHECK(dev, "device"); NULL_CHECK(first_tile_row, "first_tile_row"); NULL_CHECK(tile_row_step, "tile_row_step"); NULL_CHECK(tile_rows, "tile_rows");
    split_rows(dev->split_layout, dev->split_rank, dev->split_world, (height + TILE - 1) / TILE, first_tile_row, tile_row_step, tile_rows);
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_band_rows(mirhi_device* dev, uint32_t height, uint32_t* row_begin, uint32_t* row_end) {
    NULL_CHECK(dev, "device"); NULL_CHECK(row_begin, "row_begin"); NULL_CHECK(row_end, "row_end");
    if (dev->split_world > 1 && dev->split_layout != MIRHI_SPLIT_BANDS)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the device's tile split is interleaved (no single band of rows): use mirhi_device_split_rows");
    uint32_t first, step, count;
    split_rows(MIRHI_SPLIT_BANDS, dev->split_rank, dev->split_world, (height + TILE - 1) / TILE, &first, &step, &count);
    uint32_t p0 = first * TILE, p1 = (first + count) * TILE;
    if (p0 > height) p0 = height;
    if (p1 > height) p1 = height;
    *row_begin = p0; *row_end = p1;
    return MIRHI_OK;
}
static const char* usage_name(mirhi_buffer_usage u) {
    static const char* names[] = {"vertex", "index", "uniform", "storage", "staging", "indirect"};
    return (u >= 0 && u <= 5) ? names[u] : "unknown";
}
static bool usage_host_visible(mirhi_buffer_usage u) {   // BufferUsage::memory_location buffer.rs:86-100
    return u == MIRHI_BUFFER_VERTEX || u == MIRHI_BUFFER_INDEX || u == MIRHI_BUFFER_UNIFORM || u == MIRHI_BUFFER_STAGING;
}

extern "C" mirhi_result mirhi_buffer_create(mirhi_device* dev, mirhi_buffer_usage usage, uint64_t size, mirhi_buffer** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    *out = nullptr;
    if ((int)usage < 0 || (int)usage > 5) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown buffer usage %d", (int)usage);
    if (size == 0) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Buffer size must be greater than 0");   // buffer.rs:150-154
    HIP_TRY(hipSetDevice(dev->ordinal));
    void* p = nullptr;
    // Uniform buffers are what a frame loop rewrites every frame (Buffer::write_data on mapped memory, buffer.rs:247-279): like the
    // parameter block they live in fine-grained device memory that the host writes with plain stores (0.2 us per KB, no HIP call).
    // MIRHI_PARAM_UPLOAD=copy (or a refused allocation) keeps them in plain device memory behind copies.
    const char* upload = getenv("MIRHI_PARAM_UPLOAD");
    const bool want_copy = upload && strcmp(upload, "copy") == 0;
    bool direct = false;
    hipError_t e = hipErrorNotSupported;
    if (usage == MIRHI_BUFFER_UNIFORM && size <= (1u << 20) && !want_copy) {
        e = hipExtMallocWithFlags(&p, (size + 255) & ~(uint64_t)255, hipDeviceMallocFinegrained);
        direct = e == hipSuccess;
        if (!direct) (void)hipGetLastError();
    }
    if (!direct) e = hipMalloc(&p, (size + 255) & ~(uint64_t)255);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc(%llu) for %s buffer: %s", (unsigned long long)size, usage_name(usage), hipGetErrorString(e)); }
    mirhi_buffer* b = new (std::nothrow) mirhi_buffer{dev, usage, size, (uint8_t*)p, true};
    if (!b) { (void)hipFree(p); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed"); }
    b->host_direct = direct;
    dev->children++;
    *out = b;
    return MIRHI_OK;
}
// Waits for the submissions that may still READ `buf` -- and for no others: the command buffers whose recording names memory inside the
// buffer and that are pending.  (In the reference the memory is mapped and write_data is a memcpy: not writing what a frame in flight
// reads is the caller's business, which is why it keeps one uniform buffer per frame in flight.  A frame loop that has waited for its
// slot's fence finds nothing pending here; a caller that has not is made to wait for exactly the frames concerned.)
static mirhi_result settle_pending(mirhi_cmd* cmd, bool in_submit = false);
static mirhi_result settle_readers(mirhi_device* dev, const uint8_t* lo, const uint8_t* hi);
extern "C" mirhi_result mirhi_buffer_write(mirhi_buffer* buf, uint64_t offset, const void* data, uint64_t len) {
    NULL_CHECK(buf, "buffer");
    if (len == 0) return MIRHI_OK;                                                        // buffer.rs:248-250
    NULL_CHECK(data, "data");
    if (offset + len > buf->size || offset + len < offset)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Write exceeds buffer size: offset %llu + data %llu > buffer %llu",
                    (unsigned long long)offset, (unsigned long long)len, (unsigned long long)buf->size);   // buffer.rs:252-260
    if (!usage_host_visible(buf->usage))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Buffer memory is not mapped");              // buffer.rs:266-268
    // host-coherent write semantics: ordered after the submitted work that reads the buffer, visible to later submits
    { mirhi_result r0 = settle_readers(buf->dev, buf->ptr, buf->ptr + buf->size); if (r0 != MIRHI_OK) return r0; }
    if (buf->host_direct) {
        memcpy(buf->ptr + offset, data, len);           // write-combined stores over the BAR ...
        __builtin_ia32_sfence();                          // ... out of the write-combining buffers before a later submit rings a doorbell
        return MIRHI_OK;
    }
    HIP_TRY(hipSetDevice(buf->dev->ordinal));
    buf->dev->foreign_writes++;
    HIP_TRY(hipMemcpyAsync(buf->ptr + offset, data, len, hipMemcpyHostToDevice, buf->dev->stream));
    HIP_TRY(hipStreamSynchronize(buf->dev->stream));
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_buffer_upload(mirhi_buffer* buf, const void* data, uint64_t len) { return mirhi_buffer_write(buf, 0, data, len); }
extern "C" mirhi_result mirhi_buffer_upload_via_staging(mirhi_buffer* buf, const void* data, uint64_t len) {
    NULL_CHECK(buf, "buffer");
    if (len == 0) return MIRHI_OK;
    NULL_CHECK(data, "data");
    if (len > buf->size)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Upload exceeds buffer size: data %llu > buffer %llu", (unsigned long long)len, (unsigned long long)buf->size);
    { mirhi_result r0 = sync_all_lanes(buf->dev); if (r0 != MIRHI_OK) return r0; }
    buf->dev->foreign_writes++;
    HIP_TRY(hipMemcpyAsync(buf->ptr, data, len, hipMemcpyHostToDevice, buf->dev->stream));
    HIP_TRY(hipStreamSynchronize(buf->dev->stream));
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_buffer_create_with_data(mirhi_device* dev, mirhi_buffer_usage usage, const void* data, uint64_t len, mirhi_buffer** out) {
    mirhi_result r = mirhi_buffer_create(dev, usage, len, out);                           // buffer.rs:227-231
    if (r != MIRHI_OK) return r;
    r = mirhi_buffer_write(*out, 0, data, len);
    if (r != MIRHI_OK) { std::string keep = g_last_error; mirhi_buffer_destroy(*out); *out = nullptr; g_last_error = keep; }
    return r;
}
extern "C" mirhi_result mirhi_buffer_wrap_device_memory(mirhi_device* dev, mirhi_buffer_usage usage, void* device_ptr, uint64_t size, mirhi_buffer** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (size == 0 || !device_ptr) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Buffer size must be greater than 0");
    mirhi_buffer* b = new (std::nothrow) mirhi_buffer{dev, usage, size, (uint8_t*)device_ptr, false};
    if (!b) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    dev->foreign_writes++;
    dev->children++;
    *out = b;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_buffer_read(mirhi_buffer* buf, uint64_t offset, void* dst, uint64_t len) {
    NULL_CHECK(buf, "buffer");
    if (len == 0) return MIRHI_OK;
    NULL_CHECK(dst, "dst");
    if (offset + len > buf->size || offset + len < offset)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Read exceeds buffer size: offset %llu + len %llu > buffer %llu",
                    (unsigned long long)offset, (unsigned long long)len, (unsigned long long)buf->size);
    { mirhi_result r0 = sync_all_lanes(buf->dev); if (r0 != MIRHI_OK) return r0; }
    HIP_TRY(hipMemcpyAsync(dst, buf->ptr + offset, len, hipMemcpyDeviceToHost, buf->dev->stream));
    HIP_TRY(hipStreamSynchronize(buf->dev->stream));
    return MIRHI_OK;
}
extern "C" uint64_t mirhi_buffer_size(const mirhi_buffer* buf) { return buf ? buf->size : 0; }
extern "C" int32_t mirhi_buffer_usage_of(const mirhi_buffer* buf) { return buf ? (int32_t)buf->usage : -1; }
extern "C" void* mirhi_buffer_device_ptr(const mirhi_buffer* buf) { return buf ? buf->ptr : nullptr; }
extern "C" mirhi_result mirhi_buffer_destroy(mirhi_buffer* buf) {
    NULL_CHECK(buf, "buffer");
    (void)hipSetDevice(buf->dev->ordinal);
    if (buf->owned) { (void)sync_all_lanes(buf->dev); (void)hipFree(buf->ptr); }
    buf->dev->children--;
    delete buf;
    return MIRHI_OK;
}

// ------------------------------------------------------------------------------------------------
// images
// ------------------------------------------------------------------------------------------------
#include "mirhi_ibl.hip.h"   // cube layout (ibl_level_offset) and the IBL precompute kernels, launched further down beside mip_kernel
// a multisampled image where only an image with memory will do; what: what the caller would have done with it
static mirhi_result refuse_multisampled(const mirhi_image* img, const char* what) {
    if (img && img->samples != 1u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a multisampled image is a transient attachment without memory: it cannot be %s", what);
    return MIRHI_OK;
}
#define REFUSE_MULTISAMPLED(img, what) do { mirhi_result rm__ = refuse_multisampled((img), (what)); if (rm__ != MIRHI_OK) return rm__; } while (0)
static mirhi_result image_common(mirhi_device* dev, uint32_t w, uint32_t h, mirhi_format f, void* ext, mirhi_image** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (w == 0 || h == 0)   // depth_buffer.rs:118-127
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Image dimensions must be greater than 0 (got %ux%u)", w, h);
    if (w > 16384 || h > 16384) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Image dimensions exceed 16384 (got %ux%u)", w, h);
    const uint32_t bpp = format_bpp(f);
    if (bpp == 0) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported image format %d", (int)f);
    void* p = ext;
    if (!ext) {
        HIP_TRY(hipSetDevice(dev->ordinal));
        hipError_t e = hipMalloc(&p, (size_t)w * h * bpp);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc for %ux%u image: %s", w, h, hipGetErrorString(e)); }
    }
    mirhi_image* img = new (std::nothrow) mirhi_image{dev, w, h, f, (uint8_t*)p, ext == nullptr};
    if (!img) { if (!ext) (void)hipFree(p); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed"); }
    { std::lock_guard<std::mutex> lock(dev->mu); dev->images.push_back(img); }
    dev->children++;
    *out = img;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_image_create(mirhi_device* dev, uint32_t w, uint32_t h, mirhi_format f, mirhi_image** out) { return image_common(dev, w, h, f, nullptr, out); }
extern "C" mirhi_result mirhi_image_wrap_device_memory(mirhi_device* dev, uint32_t w, uint32_t h, mirhi_format f, void* ptr, mirhi_image** out) {
    if (!ptr) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: device_ptr is null");
    if (dev) dev->foreign_writes++;
    return image_common(dev, w, h, f, ptr, out);
}
extern "C" mirhi_result mirhi_image_create_multisampled(mirhi_device* dev, uint32_t w, uint32_t h, mirhi_format f, uint32_t samples, mirhi_image** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (const char* why = msaa_sample_count_refusal(samples)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s (got %u)", why, samples);
    if (w == 0 || h == 0) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Image dimensions must be greater than 0 (got %ux%u)", w, h);
    if (w > 16384 || h > 16384) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Image dimensions exceed 16384 (got %ux%u)", w, h);
    if (f != MIRHI_FORMAT_B8G8R8A8_SRGB && f != MIRHI_FORMAT_R32G32B32A32_SFLOAT && f != MIRHI_FORMAT_D32_SFLOAT)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: multisampled images of format %d (B8G8R8A8_SRGB, R32G32B32A32_SFLOAT or D32_SFLOAT)", (int)f);
    mirhi_image* img = new (std::nothrow) mirhi_image{dev, w, h, f, nullptr, false};      // (transient: no memory)
    if (!img) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    img->samples = samples;
    { std::lock_guard<std::mutex> lock(dev->mu); dev->images.push_back(img); }
    dev->children++;
    *out = img;
    return MIRHI_OK;
}
extern "C" uint32_t mirhi_image_samples(const mirhi_image* img) { return img ? img->samples : 0; }
extern "C" uint32_t mirhi_image_width(const mirhi_image* img) { return img ? img->width : 0; }
extern "C" uint32_t mirhi_image_height(const mirhi_image* img) { return img ? img->height : 0; }
extern "C" int32_t mirhi_image_format(const mirhi_image* img) { return img ? (int32_t)img->format : 0; }
extern "C" uint64_t mirhi_image_size_bytes(const mirhi_image* img) {
    if (!img) return 0;
    if (img->samples != 1u) return 0;      // (a multisampled image is transient: it owns no memory)
    if (img->is_cube) return (uint64_t)ibl_chain_texels(img->width, img->levels) * format_bpp(img->format);       // the whole chain
    return (uint64_t)img->width * img->height * format_bpp(img->format) * img->layers;
}
extern "C" uint32_t mirhi_image_layers(const mirhi_image* img) { return img ? img->layers : 0; }
// Texture2DArray<float> (model_pbr_ibl_csm.hlsl:115-116): one allocation, layer k at byte offset k * width * height * bpp
extern "C" mirhi_result mirhi_image_create_array(mirhi_device* dev, uint32_t w, uint32_t h, uint32_t layers, mirhi_format f, mirhi_image** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (w == 0 || h == 0) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Image dimensions must be greater than 0 (got %ux%u)", w, h);
    if (w > 16384 || h > 16384) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: Image dimensions exceed 16384 (got %ux%u)", w, h);
    if (layers == 0 || layers > 2048u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: array layers must be in [1, 2048] (got %u)", layers);
    if (f != MIRHI_FORMAT_D32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: array images of format %d (D32_SFLOAT only)", (int)f);
    const uint64_t bytes = (uint64_t)w * h * format_bpp(f) * layers;
    if (bytes > (1ull << 32)) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: %ux%u x %u layers exceeds 4 GiB", w, h, layers);   // (texel offsets stay 32-bit in the kernels)
    HIP_TRY(hipSetDevice(dev->ordinal));
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc for %ux%u x %u image array: %s", w, h, layers, hipGetErrorString(e)); }
    mirhi_image* img = new (std::nothrow) mirhi_image{dev, w, h, f, (uint8_t*)p, true};
    if (!img) { (void)hipFree(p); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed"); }
    img->layers = layers; img->is_array = true;
    { std::lock_guard<std::mutex> lock(dev->mu); dev->images.push_back(img); }
    dev->children++;
    *out = img;
    return MIRHI_OK;
}
// VkImageView with baseArrayLayer = layer, layerCount = 1 (what DepthAttachment takes, rendering.rs:319-370)
extern "C" mirhi_result mirhi_image_create_layer_view(mirhi_image* array, uint32_t layer, mirhi_image** out) {
    NULL_CHECK(array, "image"); NULL_CHECK(out, "out");
    *out = nullptr;
    REFUSE_MULTISAMPLED(array, "viewed by layer");
    if (array->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image has no layer views");
    if (!array->is_array) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: layer views are made of array images (mirhi_image_create_array)");
    if (layer >= array->layers) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: layer %u out of range (the array has %u layers)", layer, array->layers);
    mirhi_device* dev = array->dev;
    uint8_t* p = array->ptr + (size_t)layer * array->width * array->height * format_bpp(array->format);
    mirhi_image* img = new (std::nothrow) mirhi_image{dev, array->width, array->height, array->format, p, false};
    if (!img) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    img->parent = array;
    { std::lock_guard<std::mutex> lock(dev->mu); dev->images.push_back(img); array->views++; }
    dev->children++;
    *out = img;
    return MIRHI_OK;
}
extern "C" void* mirhi_image_device_ptr(const mirhi_image* img) { return img ? img->ptr : nullptr; }
extern "C" mirhi_result mirhi_image_upload(mirhi_image* img, const void* src, uint64_t len) {
    NULL_CHECK(img, "image"); NULL_CHECK(src, "src");
    REFUSE_MULTISAMPLED(img, "uploaded to");
    if (len != mirhi_image_size_bytes(img))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: image upload size %llu != image size %llu", (unsigned long long)len, (unsigned long long)mirhi_image_size_bytes(img));
    { mirhi_result r0 = sync_all_lanes(img->dev); if (r0 != MIRHI_OK) return r0; }
    img->dev->foreign_writes++;
    HIP_TRY(hipMemcpyAsync(img->ptr, src, len, hipMemcpyHostToDevice, img->dev->stream));
    HIP_TRY(hipStreamSynchronize(img->dev->stream));
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_image_read(mirhi_image* img, void* dst, uint64_t len) {
    NULL_CHECK(img, "image"); NULL_CHECK(dst, "dst");
    REFUSE_MULTISAMPLED(img, "read");
    if (len != mirhi_image_size_bytes(img))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: image read size %llu != image size %llu", (unsigned long long)len, (unsigned long long)mirhi_image_size_bytes(img));
    { mirhi_result r0 = sync_all_lanes(img->dev); if (r0 != MIRHI_OK) return r0; }
    HIP_TRY(hipMemcpyAsync(dst, img->ptr, len, hipMemcpyDeviceToHost, img->dev->stream));
    HIP_TRY(hipStreamSynchronize(img->dev->stream));
    return MIRHI_OK;
}
// one thread per texel of the destination level: 2x2 box filter on the stored bytes, round half up, edge clamp
__global__ void mip_kernel(const uint32_t* __restrict__ src, uint32_t sw, uint32_t sh, uint32_t* __restrict__ dst, uint32_t dw, uint32_t dh) {
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= dw || y >= dh) return;
    const uint32_t x0 = 2u * x < sw ? 2u * x : sw - 1u, x1 = 2u * x + 1u < sw ? 2u * x + 1u : sw - 1u;
    const uint32_t y0 = 2u * y < sh ? 2u * y : sh - 1u, y1 = 2u * y + 1u < sh ? 2u * y + 1u : sh - 1u;
    const uint32_t a = src[y0 * sw + x0], b = src[y0 * sw + x1], c = src[y1 * sw + x0], e = src[y1 * sw + x1];
    uint32_t out = 0;
    for (uint32_t sft = 0; sft < 32u; sft += 8u)
        out |= ((((a >> sft) & 0xFFu) + ((b >> sft) & 0xFFu) + ((c >> sft) & 0xFFu) + ((e >> sft) & 0xFFu) + 2u) >> 2) << sft;
    dst[y * dw + x] = out;
}
extern "C" uint32_t mirhi_image_mip_levels(const mirhi_image* img) { return img ? img->levels : 0; }
extern "C" mirhi_result mirhi_image_generate_mips(mirhi_image* img) {
    NULL_CHECK(img, "image");
    REFUSE_MULTISAMPLED(img, "given a mip chain");
    if (img->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image's mip chain is built by mirhi_ibl_cube_generate_mips");
    if (img->format != MIRHI_FORMAT_R8G8B8A8_UNORM && img->format != MIRHI_FORMAT_R8G8B8A8_SRGB)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: mip chains are built for R8G8B8A8 textures only");
    if (!img->owned) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: cannot grow a wrapped image into a mip chain");
    HIP_TRY(hipSetDevice(img->dev->ordinal));
    { mirhi_result r0 = sync_all_lanes(img->dev); if (r0 != MIRHI_OK) return r0; }
    uint32_t levels = 1;
    size_t texels = (size_t)img->width * img->height;
    for (uint32_t w = img->width, h = img->height; w > 1 || h > 1; levels++) { w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1; texels += (size_t)w * h; }
    uint8_t* chain = img->ptr;
    if (img->levels != levels) {              // first call: move level 0 into a buffer that holds the whole chain
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, texels * 4);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc for a %zu-texel mip chain: %s", texels, hipGetErrorString(e)); }
        chain = (uint8_t*)p;
        img->dev->foreign_writes++;
        HIP_TRY(hipMemcpyAsync(chain, img->ptr, (size_t)img->width * img->height * 4, hipMemcpyDeviceToDevice, img->dev->stream));
    }
    uint32_t sw = img->width, sh = img->height;
    uint32_t* src = (uint32_t*)chain;
    for (uint32_t l = 1; l < levels; l++) {
        const uint32_t dw = sw > 1 ? sw >> 1 : 1, dh = sh > 1 ? sh >> 1 : 1;
        uint32_t* dst = src + (size_t)sw * sh;
        hipLaunchKernelGGL(mip_kernel, dim3((dw + 63) / 64, dh), dim3(64), 0, img->dev->stream, src, sw, sh, dst, dw, dh);
        HIP_TRY(hipGetLastError());
        src = dst; sw = dw; sh = dh;
    }
    HIP_TRY(hipStreamSynchronize(img->dev->stream));
    if (chain != img->ptr) { (void)hipFree(img->ptr); img->ptr = chain; }
    img->levels = levels;
    return MIRHI_OK;
}
// ------------------------------------------------------------------------------------------------
// cube images and the IBL precompute passes (kernels: mirhi_ibl.hip.h; include/mirhi.h "IBL precompute")
// ------------------------------------------------------------------------------------------------
extern "C" mirhi_result mirhi_image_create_cube(mirhi_device* dev, uint32_t size, uint32_t levels, mirhi_format f, mirhi_image** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (f != MIRHI_FORMAT_R32G32B32A32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: cube images of format %d (R32G32B32A32_SFLOAT only)", (int)f);
    if (size == 0 || size > 4096u || (size & (size - 1u))) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube's size must be a power of two in [1, 4096] (got %u)", size);
    uint32_t full = 1; while ((size >> full) != 0u) full++;                       // log2(size) + 1
    if (levels == 0 || levels > full) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a %u^2 cube has 1 to %u mip levels (got %u)", size, full, levels);
    const uint64_t bytes = (uint64_t)ibl_chain_texels(size, levels) * 16u;         // (at most 8 * 4096^2 texels: texel offsets stay 32-bit in the kernels)
    HIP_TRY(hipSetDevice(dev->ordinal));
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, (size_t)bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc for a %u^2 cube of %u levels: %s", size, levels, hipGetErrorString(e)); }
    mirhi_image* img = new (std::nothrow) mirhi_image{dev, size, size, f, (uint8_t*)p, true};
    if (!img) { (void)hipFree(p); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed"); }
    img->layers = 6; img->levels = levels; img->is_cube = true;
    { std::lock_guard<std::mutex> lock(dev->mu); dev->images.push_back(img); }
    dev->children++;
    *out = img;
    return MIRHI_OK;
}
static mirhi_result ibl_cube_arg(const mirhi_image* img, const char* what) {
    if (!img) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s is null", what);
    REFUSE_MULTISAMPLED(img, "an IBL pass's image");
    if (!img->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s must be a cube image (mirhi_image_create_cube)", what);
    return MIRHI_OK;
}
static mirhi_result ibl_2d_arg(const mirhi_image* img, const char* what) {
    if (!img) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s is null", what);
    REFUSE_MULTISAMPLED(img, "an IBL pass's image");
    if (img->is_cube || img->is_array || img->parent) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s must be a 2-D image", what);
    if (img->format != MIRHI_FORMAT_R32G32B32A32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s must be R32G32B32A32_SFLOAT (format %d)", what, (int)img->format);
    return MIRHI_OK;
}
static mirhi_result ibl_pair(const mirhi_image* a, const mirhi_image* b) {
    if (a == b) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a pass cannot read and write the same image");
    if (a->dev != b->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the two images belong to different devices");
    return MIRHI_OK;
}
// the frame of every pass: lost device, all lanes idle, launch on the device stream, foreign write, wait (as mirhi_image_generate_mips)
static mirhi_result ibl_begin(mirhi_device* dev) {
    if (dev->native && dev->native->lost.load(std::memory_order_acquire)) return device_lost(dev);
    HIP_TRY(hipSetDevice(dev->ordinal));
    { mirhi_result r0 = sync_all_lanes(dev); if (r0 != MIRHI_OK) return r0; }
    dev->foreign_writes++;
    return MIRHI_OK;
}
static mirhi_result ibl_end(mirhi_device* dev) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dev->stream));
    return MIRHI_OK;
}
static IblCube ibl_cube_of(const mirhi_image* img) { return IblCube{(const float4*)img->ptr, img->width, img->levels}; }

extern "C" mirhi_result mirhi_ibl_equirect_to_cube(mirhi_image* src2d, mirhi_image* cube) {
    { mirhi_result r = ibl_2d_arg(src2d, "the equirectangular source"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_cube_arg(cube, "the destination"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_pair(src2d, cube); if (r != MIRHI_OK) return r; }
    mirhi_device* dev = cube->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    const uint32_t n = cube->width, texels = 6u * n * n;
    hipLaunchKernelGGL(ibl_equirect_kernel, dim3((texels + 255u) / 256u), dim3(256), 0, dev->stream, (const float4*)src2d->ptr, src2d->width, src2d->height, (float4*)cube->ptr, n);
    return ibl_end(dev);
}
// a Radiance RGBE source: an ordinary 2-D R8G8B8A8_UNORM image whose bytes are (R, G, B, E); with a mip chain, level 0 is read
static mirhi_result rgbe_source_arg(const mirhi_image* img) {
    if (!img) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the RGBE source is null");
    if (img->samples != 1u || img->is_cube || img->is_array || img->parent) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the RGBE source must be a 2-D image");
    if (img->format != MIRHI_FORMAT_R8G8B8A8_UNORM)      // (R8G8B8A8_SRGB too: the bytes are no colours)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the RGBE source must be R8G8B8A8_UNORM (format %d)", (int)img->format);
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_image_expand_rgbe(mirhi_image* rgbe8, mirhi_image* dst) {
    { mirhi_result r = rgbe_source_arg(rgbe8); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_2d_arg(dst, "the destination"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_pair(rgbe8, dst); if (r != MIRHI_OK) return r; }
    if (dst->width != rgbe8->width || dst->height != rgbe8->height)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the destination must have the source's extent (%ux%u, got %ux%u)", rgbe8->width, rgbe8->height, dst->width, dst->height);
    mirhi_device* dev = dst->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    const uint32_t texels = dst->width * dst->height;          // (at most 16384^2 = 2^28)
    hipLaunchKernelGGL(rgbe_expand_kernel, dim3((texels + RGBE_EXPAND_PER_BLOCK - 1u) / RGBE_EXPAND_PER_BLOCK), dim3(256), 0, dev->stream, (const uint32_t*)rgbe8->ptr, (float4*)dst->ptr, texels);
    return ibl_end(dev);
}
extern "C" mirhi_result mirhi_ibl_equirect_to_cube_rgbe(mirhi_image* rgbe8, mirhi_image* cube) {
    { mirhi_result r = rgbe_source_arg(rgbe8); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_cube_arg(cube, "the destination"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_pair(rgbe8, cube); if (r != MIRHI_OK) return r; }
    mirhi_device* dev = cube->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    const uint32_t n = cube->width, texels = 6u * n * n;
    hipLaunchKernelGGL(ibl_equirect_rgbe_kernel, dim3((texels + 255u) / 256u), dim3(256), 0, dev->stream, (const uint32_t*)rgbe8->ptr, rgbe8->width, rgbe8->height, (float4*)cube->ptr, n);
    return ibl_end(dev);
}
extern "C" mirhi_result mirhi_ibl_cube_generate_mips(mirhi_image* cube) {
    { mirhi_result r = ibl_cube_arg(cube, "the image"); if (r != MIRHI_OK) return r; }
    mirhi_device* dev = cube->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    for (uint32_t l = 1; l < cube->levels; l++) {
        const uint32_t dn = cube->width >> l, texels = 6u * dn * dn;
        hipLaunchKernelGGL(ibl_cube_mip_kernel, dim3((texels + 255u) / 256u), dim3(256), 0, dev->stream,
                           (const float4*)cube->ptr + ibl_level_offset(cube->width, l - 1u), (float4*)cube->ptr + ibl_level_offset(cube->width, l), dn);
        HIP_TRY(hipGetLastError());
    }
    return ibl_end(dev);
}
extern "C" mirhi_result mirhi_ibl_irradiance(mirhi_image* env, mirhi_image* out) {
    { mirhi_result r = ibl_cube_arg(env, "the environment"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_cube_arg(out, "the destination"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_pair(env, out); if (r != MIRHI_OK) return r; }
    mirhi_device* dev = out->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    const uint32_t n = out->width;
    if (env->cube_seamless) hipLaunchKernelGGL(ibl_irradiance_kernel_seamless, dim3(6u * n * n), dim3(256), 0, dev->stream, ibl_cube_of(env), (float4*)out->ptr, n);
    else hipLaunchKernelGGL(ibl_irradiance_kernel, dim3(6u * n * n), dim3(256), 0, dev->stream, ibl_cube_of(env), (float4*)out->ptr, n);
    return ibl_end(dev);
}
extern "C" mirhi_result mirhi_ibl_prefilter(mirhi_image* env, mirhi_image* out, uint32_t sample_count) {
    { mirhi_result r = ibl_cube_arg(env, "the environment"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_cube_arg(out, "the destination"); if (r != MIRHI_OK) return r; }
    { mirhi_result r = ibl_pair(env, out); if (r != MIRHI_OK) return r; }
    if (sample_count == 0 || sample_count > 4096u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: sample_count must be in [1, 4096] (got %u)", sample_count);
    mirhi_device* dev = out->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    IblPrefilterPlan plan{};
    plan.levels = out->levels; plan.sample_count = sample_count; plan.size = out->width;     // (levels <= 13 = IBL_MAX_LEVELS: size <= 4096)
    uint32_t blocks = 0;
    for (uint32_t l = 0; l < out->levels; l++) {
        const uint32_t m = out->width >> l, texels = 6u * m * m;
        const bool mirror = out->levels == 1u || (float)l / (float)(out->levels - 1u) < 0.01f;
        uint32_t lanes = 1;                         // split a texel's samples over 4, 16 or 64 lanes while the level has fewer than 128 Ki threads
        while (!mirror && lanes < 64u && texels * lanes < 131072u) lanes *= 4u;
        plan.first_block[l] = blocks; plan.lanes[l] = lanes;
        blocks += (texels + 256u / lanes - 1u) / (256u / lanes);
    }
    plan.first_block[out->levels] = blocks;
    if (env->cube_seamless) hipLaunchKernelGGL(ibl_prefilter_kernel_seamless, dim3(blocks), dim3(256), (size_t)sample_count * sizeof(float4), dev->stream, ibl_cube_of(env), (float4*)out->ptr, plan);
    else hipLaunchKernelGGL(ibl_prefilter_kernel, dim3(blocks), dim3(256), (size_t)sample_count * sizeof(float4), dev->stream, ibl_cube_of(env), (float4*)out->ptr, plan);
    return ibl_end(dev);
}
extern "C" mirhi_result mirhi_ibl_brdf_lut(mirhi_image* out2d) {
    { mirhi_result r = ibl_2d_arg(out2d, "the destination"); if (r != MIRHI_OK) return r; }
    if (out2d->width != out2d->height) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the BRDF LUT must be square (got %ux%u)", out2d->width, out2d->height);
    if (out2d->levels != 1u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the BRDF LUT must have no mip chain");
    mirhi_device* dev = out2d->dev;
    { mirhi_result r = ibl_begin(dev); if (r != MIRHI_OK) return r; }
    const uint32_t n = out2d->width;
    hipLaunchKernelGGL(ibl_brdf_lut_kernel, dim3((n + 255u) / 256u, n), dim3(256), 0, dev->stream, (float4*)out2d->ptr, n);
    return ibl_end(dev);
}
extern "C" uint32_t mirhi_image_max_anisotropy(const mirhi_image* img) { return img ? img->max_anisotropy : 0; }
extern "C" mirhi_result mirhi_image_set_max_anisotropy(mirhi_image* img, uint32_t max_anisotropy) {
    NULL_CHECK(img, "image");
    REFUSE_MULTISAMPLED(img, "sampled (it has no sampler state)");
    if (img->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image has no anisotropic sampler (the cube sampler is fixed, include/mirhi.h)");
    if (img->format != MIRHI_FORMAT_R8G8B8A8_UNORM && img->format != MIRHI_FORMAT_R8G8B8A8_SRGB)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: anisotropic filtering applies to sampled R8G8B8A8 textures only");
    if (max_anisotropy < 1u || max_anisotropy > 16u)
        return fail(MIRHI_ERR_DEVICE, "Vulkan error: maxAnisotropy %u outside [1, 16] (maxSamplerAnisotropy)", max_anisotropy);
    img->max_anisotropy = max_anisotropy;        // read when a draw is recorded, like the mip chain
    return MIRHI_OK;
}
extern "C" void mirhi_sampler_desc_default(mirhi_sampler_desc* desc) { if (desc) *desc = mirhi_sampler_desc{0, 0, 0, 0, 0}; }
extern "C" mirhi_result mirhi_image_set_sampler(mirhi_image* img, const mirhi_sampler_desc* desc) {
    NULL_CHECK(img, "image");
    NULL_CHECK(desc, "sampler desc");
    REFUSE_MULTISAMPLED(img, "sampled (it has no sampler state)");
    if (img->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image has no sampler state (the cube sampler is fixed, include/mirhi.h)");
    if (img->is_array || img->parent)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: an image array and its layer views have no sampler state (the shadow comparison sampler is fixed, include/mirhi.h)");
    if (img->format != MIRHI_FORMAT_R8G8B8A8_UNORM && img->format != MIRHI_FORMAT_R8G8B8A8_SRGB)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: sampler state applies to sampled R8G8B8A8 textures only");
    const struct { const char* name; int32_t value, count; } fields[5] = {
        {"address_u", desc->address_u, 3}, {"address_v", desc->address_v, 3}, {"mag_filter", desc->mag_filter, 2}, {"min_filter", desc->min_filter, 2}, {"mip_mode", desc->mip_mode, 3}};
    for (const auto& f : fields)
        if (f.value < 0 || f.value >= f.count) return fail(MIRHI_ERR_DEVICE, "Vulkan error: sampler %s %d outside its enum [0, %d]", f.name, f.value, f.count - 1);
    img->sampler = *desc;        // read when a draw is recorded, like max_anisotropy
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_image_set_cube_seamless(mirhi_image* cube, uint32_t enable) {
    NULL_CHECK(cube, "image");
    REFUSE_MULTISAMPLED(cube, "sampled (it has no sampler state)");
    if (!cube->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: not a cube image: seamless filtering is the state of a cube (mirhi_image_create_cube)");
    if (enable > 1u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: cube seamless state %u is neither 0 nor 1", enable);
    cube->cube_seamless = enable;      // read when a draw is recorded, like the sampler state of a texture; by the precompute passes when they are called
    return MIRHI_OK;
}
extern "C" uint32_t mirhi_image_cube_seamless(const mirhi_image* img) { return (img && img->is_cube) ? img->cube_seamless : 0u; }
extern "C" mirhi_result mirhi_image_sampler(const mirhi_image* img, mirhi_sampler_desc* out) {
    NULL_CHECK(img, "image");
    NULL_CHECK(out, "sampler desc");
    *out = img->sampler;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_image_destroy(mirhi_image* img) {
    NULL_CHECK(img, "image");
    if (img->views != 0) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: image array still has %u live layer views", img->views);
    (void)hipSetDevice(img->dev->ordinal);
    if (img->owned) { (void)sync_all_lanes(img->dev); (void)hipFree(img->ptr); }
    { std::lock_guard<std::mutex> lock(img->dev->mu); auto& v = img->dev->images; v.erase(std::remove(v.begin(), v.end(), img), v.end());
      if (img->parent) img->parent->views--; }      // (a view frees nothing)
    img->dev->children--;
    delete img;
    return MIRHI_OK;
}

// ------------------------------------------------------------------------------------------------
// pipeline (pipeline.rs:645-698 defaults, :918-952 validation)
// ------------------------------------------------------------------------------------------------
extern "C" void mirhi_pipeline_desc_default(mirhi_pipeline_desc* d) {
    if (!d) return;
    memset(d, 0, sizeof *d);
    d->vertex_program = MIRHI_PROGRAM_NONE;
    d->fragment_program = MIRHI_PROGRAM_NONE;
    d->topology = MIRHI_TOPOLOGY_TRIANGLE_LIST;
    d->polygon_mode = MIRHI_POLYGON_FILL;
    d->cull_mode = MIRHI_CULL_BACK;
    d->front_face = MIRHI_FRONT_FACE_COUNTER_CLOCKWISE;
    d->rasterization_samples = 1;
    d->depth_test_enable = 1;
    d->depth_write_enable = 1;
    d->depth_compare_op = MIRHI_COMPARE_LESS;
    d->depth_attachment_format = MIRHI_FORMAT_UNDEFINED;
    d->src_color_blend_factor = MIRHI_BLEND_ONE; d->dst_color_blend_factor = MIRHI_BLEND_ZERO; d->color_blend_op = MIRHI_BLEND_OP_ADD;   // pipeline.rs:499-512
    d->src_alpha_blend_factor = MIRHI_BLEND_ONE; d->dst_alpha_blend_factor = MIRHI_BLEND_ZERO; d->alpha_blend_op = MIRHI_BLEND_OP_ADD;
    d->color_write_mask = 0xFu;
}

// bias: the factors of a depth_bias_enable pipeline (the desc's word is set by the caller)
static mirhi_result pipeline_create(mirhi_device* dev, const mirhi_pipeline_desc* d, const mirhi_depth_bias& bias, mirhi_pipeline** out) {
    // --- the reference's own validation, same order and text (pipeline.rs:920-952) ---
    if (d->vertex_program == MIRHI_PROGRAM_NONE) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: Vertex shader is required");
    if (d->fragment_program == MIRHI_PROGRAM_NONE) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: Fragment shader is required");
    if (d->color_attachment_count == 0) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: At least one color attachment format is required");
    const bool has_depth = d->depth_attachment_format != MIRHI_FORMAT_UNDEFINED;
    if ((d->depth_test_enable || d->depth_write_enable) && !has_depth)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: Depth test or write is enabled but no depth attachment format is specified");
    if (d->blend_attachment_count != 0 && d->blend_attachment_count != d->color_attachment_count)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: Blend attachment count (%u) must match color attachment count (%u)", d->blend_attachment_count, d->color_attachment_count);
    // --- program selection replaces SPIR-V module creation (shader.rs:244-330) ---
    if (d->vertex_program < 0 || d->vertex_program > MIRHI_PROGRAM_SKYBOX || d->fragment_program < 0 || d->fragment_program > MIRHI_PROGRAM_SKYBOX)
        return fail(MIRHI_ERR_SHADER, "Shader error: unknown program id (vertex %d, fragment %d)", d->vertex_program, d->fragment_program);
    const bool vs_shadow = d->vertex_program == MIRHI_PROGRAM_SHADOW, fs_shadow = d->fragment_program == MIRHI_PROGRAM_SHADOW;
    const bool vs_model = d->vertex_program != MIRHI_PROGRAM_TRIANGLE, fs_model = d->fragment_program != MIRHI_PROGRAM_TRIANGLE;
    const bool vs_sky = d->vertex_program == MIRHI_PROGRAM_SKYBOX, fs_sky = d->fragment_program == MIRHI_PROGRAM_SKYBOX;
    if (vs_model != fs_model || vs_shadow != fs_shadow || vs_sky != fs_sky)
        return fail(MIRHI_ERR_SHADER, "Shader error: vertex program %d does not produce the inputs of fragment program %d", d->vertex_program, d->fragment_program);
    // --- what this rasterizer does not implement fails loudly instead of rendering something else ---
    if (d->color_attachment_count != 1) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: %u color attachments (exactly 1 supported)", d->color_attachment_count);
    const int32_t cf = d->color_attachment_formats[0];
    // depth-only pipelines (pixel/shadow.hlsl writes no colour): the one location holds no attachment (UNDEFINED), and only those
    if (vs_shadow && cf != MIRHI_FORMAT_UNDEFINED)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: the SHADOW program is depth-only: color attachment format must be UNDEFINED, got %d", cf);
    if (!vs_shadow && cf == MIRHI_FORMAT_UNDEFINED)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: color attachment format UNDEFINED (no attachment) is only supported for the depth-only SHADOW program");
    if (!vs_shadow && cf != MIRHI_FORMAT_B8G8R8A8_SRGB && cf != MIRHI_FORMAT_R32G32B32A32_SFLOAT)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported color attachment format %d", cf);
    if (vs_shadow) {
        const int32_t op = d->depth_compare_op;
        if (!d->depth_test_enable || !d->depth_write_enable || !ordering_compare((uint32_t)op))
            return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: depth-only pipelines need depth test and write with LESS, LESS_OR_EQUAL, GREATER or GREATER_OR_EQUAL");
        if (d->blend_enable || d->fragment_discard_enable)
            return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: blending or fragment discard in a depth-only pipeline");
    }
    if (has_depth && d->depth_attachment_format != MIRHI_FORMAT_D32_SFLOAT)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported depth attachment format %d (D32_SFLOAT only)", d->depth_attachment_format);
    if (d->topology != MIRHI_TOPOLOGY_TRIANGLE_LIST) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported topology %d (TriangleList only)", d->topology);
    if (d->polygon_mode != MIRHI_POLYGON_FILL) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported polygon mode %d (Fill only)", d->polygon_mode);
    if (d->cull_mode < 0 || d->cull_mode > 3 || d->front_face < 0 || d->front_face > 1) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: invalid cull mode / front face");
    if (d->depth_compare_op < 0 || d->depth_compare_op > 7) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: invalid depth compare op %d", d->depth_compare_op);
    if (d->rasterization_samples != 1 && d->rasterization_samples != 4) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported sample count %u", d->rasterization_samples);
    if (d->blend_enable) {
        const int32_t f[4] = {d->src_color_blend_factor, d->dst_color_blend_factor, d->src_alpha_blend_factor, d->dst_alpha_blend_factor};
        for (int32_t v : f) {
            if (v < 0 || v > MIRHI_BLEND_SRC_ALPHA_SATURATE) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: invalid blend factor %d", v);
            if (v >= MIRHI_BLEND_CONSTANT_COLOR && v <= MIRHI_BLEND_ONE_MINUS_CONSTANT_ALPHA)
                return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: constant-colour blend factors (no blend constants on this path)");
        }
        if (d->color_blend_op < 0 || d->color_blend_op > MIRHI_BLEND_OP_MAX || d->alpha_blend_op < 0 || d->alpha_blend_op > MIRHI_BLEND_OP_MAX)
            return fail(MIRHI_ERR_PIPELINE, "Pipeline error: invalid blend op");
    }
    // depth bias / depth clamp: geometry-stage state of every program that has geometry
    if (d->depth_clamp_enable || d->depth_bias_enable) {
        if (!std::isfinite(bias.constant_factor) || !std::isfinite(bias.clamp) || !std::isfinite(bias.slope_factor))
            return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: depth bias factors must be finite (constant %g, clamp %g, slope %g)", (double)bias.constant_factor,
                        (double)bias.clamp, (double)bias.slope_factor);
        if (vs_sky) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: depth bias / depth clamp on a SKYBOX pipeline (its fragments have no depth of their own)");
        if (d->rasterizer_discard_enable) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: depth bias / depth clamp together with rasterizer_discard_enable");
    }
    if (vs_sky) {
        // vertex/skybox.hlsl has no vertex input (SV_VertexID alone): no binding, no attributes (a blending or discarding one is refused at the draw)
        if (d->attribute_count != 0) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: program %d (SKYBOX) has no vertex input, got %u vertex attributes", d->vertex_program, d->attribute_count);
        mirhi_pipeline* p = new (std::nothrow) mirhi_pipeline{dev, *d, bias};
        if (!p) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
        dev->children++;
        *out = p;
        return MIRHI_OK;
    }
    const uint32_t want_stride = vs_shadow ? 12u : (vs_model ? 48u : 24u);      // vertex.rs:35-41 / :130-136; vertex/shadow.hlsl:13-16 (position only)
    if (d->vertex_stride < want_stride || (d->vertex_stride & 3u))
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: vertex stride %u too small for program %d (needs >= %u, multiple of 4)", d->vertex_stride, d->vertex_program, want_stride);
    const uint32_t want_attrs = vs_shadow ? 1u : (vs_model ? 4u : 2u);
    static const uint32_t model_offsets[4] = {0, 12, 24, 32}, tri_offsets[2] = {0, 12};
    if (d->attribute_count != want_attrs) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: program %d expects %u vertex attributes, got %u", d->vertex_program, want_attrs, d->attribute_count);
    for (uint32_t i = 0; i < want_attrs; i++)
        if (d->attribute_offsets[i] != (vs_model ? model_offsets[i] : tri_offsets[i]))
            return fail(MIRHI_ERR_PIPELINE, "Pipeline error: attribute %u offset %u does not match the reference vertex layout", i, d->attribute_offsets[i]);
    mirhi_pipeline* p = new (std::nothrow) mirhi_pipeline{dev, *d, bias};
    if (!p) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    dev->children++;
    *out = p;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_pipeline_create(mirhi_device* dev, const mirhi_pipeline_desc* d, mirhi_pipeline** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(d, "desc"); NULL_CHECK(out, "out");
    *out = nullptr;
    return pipeline_create(dev, d, mirhi_depth_bias{0.0f, 0.0f, 0.0f}, out);
}
// GraphicsPipelineBuilder::depth_bias (pipeline.rs:781-788) + build: the desc with depth_bias_enable set and the three factors
extern "C" mirhi_result mirhi_pipeline_create_with_depth_bias(mirhi_device* dev, const mirhi_pipeline_desc* d, const mirhi_depth_bias* bias, mirhi_pipeline** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(d, "desc"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (!bias) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: a NULL depth bias (mirhi_pipeline_create takes pipelines without one)");
    mirhi_pipeline_desc with = *d;
    with.depth_bias_enable = 1u;
    return pipeline_create(dev, &with, *bias, out);
}
extern "C" mirhi_result mirhi_pipeline_destroy(mirhi_pipeline* p) {
    NULL_CHECK(p, "pipeline");
    p->dev->children--;
    delete p;
    return MIRHI_OK;
}

// ------------------------------------------------------------------------------------------------
// command recording (command.rs)
// ------------------------------------------------------------------------------------------------
extern "C" void mirhi_rendering_info_default(mirhi_rendering_info* i) {
    if (!i) return;
    memset(i, 0, sizeof *i);
    i->color_load_op = MIRHI_LOAD_OP_CLEAR; i->color_store_op = MIRHI_STORE_OP_STORE;       // rendering.rs:102-115
    i->clear_color[3] = 1.0f;
    i->depth_load_op = MIRHI_LOAD_OP_CLEAR; i->depth_store_op = MIRHI_STORE_OP_DONT_CARE;   // rendering.rs:356-370
    i->clear_depth = 1.0f;
}

static void free_workspace(mirhi_cmd* c) {
    Workspace& w = c->ws;
    if (w.pblock) (void)hipFree(w.pblock);
    if (w.pstage) (void)hipHostFree(w.pstage);
    w.scope_bins.free_buffers(); w.view_bins.free_buffers();
    if (w.carry_depth) (void)hipFree(w.carry_depth);
    if (w.ordered) (void)hipFree(w.ordered);
    if (w.flat_color) (void)hipFree(w.flat_color);
    if (w.prim_draw) (void)hipFree(w.prim_draw);
    if (w.stats_prim) (void)hipFree(w.stats_prim);
    if (w.stats_params) (void)hipFree(w.stats_params);
    if (w.status_host) (void)hipHostFree(w.status_host);
    w = Workspace();
}

// The device-side status of a finished submission lives in the command buffer's workspace.  Before that workspace goes away
// (destroy) or is re-armed (end() of a new recording) every fence that still lists the command buffer -- Vulkan allows
// destroying a command buffer before its fence is waited on, and the Rust wrapper's Drop order does exactly that -- takes the
// status over; so does the device's wait_idle bookkeeping.  The caller has synchronised the command buffer's lane.
static mirhi_result status_of(mirhi_device* dev, mirhi_cmd* c);
static void hand_over_status(mirhi_cmd* cmd) {
    mirhi_device* dev = cmd->dev;
    std::lock_guard<std::mutex> lock(dev->mu);
    auto& u = dev->unchecked;
    const bool was_unchecked = std::find(u.begin(), u.end(), cmd) != u.end();
    bool listed = false;
    for (mirhi_fence* f : dev->fences) listed |= std::find(f->cmds.begin(), f->cmds.end(), cmd) != f->cmds.end();
    if (!was_unchecked && !listed) return;
    const std::string keep = g_last_error;
    const mirhi_result rc = status_of(dev, cmd);
    const std::string msg = g_last_error;
    g_last_error = keep;
    for (mirhi_fence* f : dev->fences) {
        bool had = false;
        for (size_t i = f->cmds.size(); i-- > 0;)
            if (f->cmds[i] == cmd) { f->cmds.erase(f->cmds.begin() + (ptrdiff_t)i); f->seqs.erase(f->seqs.begin() + (ptrdiff_t)i); had = true; }
        if (had && rc != MIRHI_OK) { f->deferred = rc; f->deferred_msg = msg; }
    }
    if (was_unchecked) {
        u.erase(std::remove(u.begin(), u.end(), cmd), u.end());
        if (rc != MIRHI_OK && !listed) { dev->deferred = rc; dev->deferred_msg = msg; }
    }
}

extern "C" mirhi_result mirhi_cmd_create(mirhi_device* dev, mirhi_cmd** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    mirhi_cmd* c = new (std::nothrow) mirhi_cmd();
    if (!c) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    c->dev = dev;
    c->lane = dev->next_lane++ % (uint32_t)dev->lanes.size();
    { std::lock_guard<std::mutex> lock(dev->mu); dev->cmds.push_back(c); }
    dev->children++;
    *out = c;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_set_queue_lane(mirhi_cmd* cmd, uint32_t lane) {
    NULL_CHECK(cmd, "command buffer");
    if (lane >= cmd->dev->lanes.size()) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: queue lane %u of %zu", lane, cmd->dev->lanes.size());
    drain_submits(cmd->dev);
    if (!drain_native(cmd->dev, cmd->last_native)) return device_lost(cmd->dev);
    if (cmd->last_stream) HIP_TRY(hipStreamSynchronize(cmd->last_stream));
    HIP_TRY(hipStreamSynchronize(cmd->dev->lanes[cmd->lane < cmd->dev->lanes.size() ? cmd->lane : 0]));
    cmd_finished(cmd);
    cmd->lane = lane;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_destroy(mirhi_cmd* cmd) {
    NULL_CHECK(cmd, "command buffer");
    (void)sync_all_lanes(cmd->dev);
    cmd_finished(cmd);
    hand_over_status(cmd);          // fences (and wait_idle) that still list this command buffer keep its device status
    { std::lock_guard<std::mutex> lock(cmd->dev->mu); auto& v = cmd->dev->cmds; v.erase(std::remove(v.begin(), v.end(), cmd), v.end()); }
    free_workspace(cmd);
    cmd->dev->children--;
    delete cmd;
    return MIRHI_OK;
}
static void reset_recording(mirhi_cmd* c) {
    // (the launch plan and the recording it was built from stay: end() compares the new recording with it -- see mirhi_cmd::planned)
    c->passes.clear();
    c->in_rendering = false;
    c->pipeline = nullptr; c->vb = nullptr; c->ib = nullptr;
    for (auto& u : c->uniforms) u = {nullptr, 0, 0};
    for (auto& tx : c->textures) tx = nullptr;
    c->cascades = nullptr; c->cascade_params = {nullptr, 0, 0}; c->cascade_blend = 0.0f;
    for (auto& im : c->ibl) im = nullptr;
    c->skybox = nullptr;
    memset(c->push_constants, 0, sizeof c->push_constants);
    c->has_viewport = c->has_scissor = false;
}
static mirhi_result begin_common(mirhi_cmd* cmd, bool one_time) {
    NULL_CHECK(cmd, "command buffer");
    if (cmd->state == CMD_RECORDING) return fail(MIRHI_ERR_DEVICE, "Vulkan error: command buffer is already recording");
    while (cmd->queued.load(std::memory_order_acquire) > 0) cpu_relax();
    reset_recording(cmd);          // implicit reset, as with RESET_COMMAND_BUFFER pools (command.rs:89-106)
    cmd->state = CMD_RECORDING;
    cmd->one_time = one_time;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_begin(mirhi_cmd* cmd) { return begin_common(cmd, true); }
extern "C" mirhi_result mirhi_cmd_begin_reusable(mirhi_cmd* cmd) { return begin_common(cmd, false); }
extern "C" mirhi_result mirhi_cmd_reset(mirhi_cmd* cmd) {
    NULL_CHECK(cmd, "command buffer");
    while (cmd->queued.load(std::memory_order_acquire) > 0) cpu_relax();
    reset_recording(cmd);
    cmd->state = CMD_INITIAL;
    return MIRHI_OK;
}
#define REQUIRE_RECORDING(cmd)                                                                         \
    do {                                                                                               \
        NULL_CHECK(cmd, "command buffer");                                                             \
        if ((cmd)->state != CMD_RECORDING) return fail(MIRHI_ERR_DEVICE, "Vulkan error: command buffer is not in the recording state"); \
    } while (0)

// The scope's render area as ScopeHeader::area keeps it -- the full extent spelled out -- or the refusal (mirhi_scope.h render_area: the rectangle must
// lie inside the width x height attachment).  A partial one is refused on a split device (the band exchange moves whole tile rows) -- unless the caller
// takes `partial`: a multisampled and a multiview scope refuse a partial area in words and at a place of their own (msaa_ / multiview_scope_refusal).
static mirhi_result take_render_area(const mirhi_cmd* cmd, const mirhi_rendering_info* info, uint32_t width, uint32_t height, int32_t area[4], bool* partial = nullptr) {
    const RenderArea a = render_area(width, height, info->render_area);
    if (!a.valid) {
        char msg[192];
        render_area_message(msg, sizeof msg, info->render_area, width, height);
        return fail(MIRHI_ERR_INVALID_HANDLE, "%s", msg);
    }
    if (partial) *partial = a.partial;
    else if (a.partial && cmd->dev->split_world > 1) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a partial render area on a split device");
    area[0] = (int32_t)a.x; area[1] = (int32_t)a.y; area[2] = (int32_t)a.w; area[3] = (int32_t)a.h;
    return MIRHI_OK;
}
#define REQUIRE_NO_SCOPE(cmd) do { if ((cmd)->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: begin_rendering inside an active rendering scope"); } while (0)
static ScopeHeader::Target target_of(const mirhi_image* img) {
    return img ? ScopeHeader::Target{img->ptr, img->width, img->height, (uint32_t)img->format, 0u} : ScopeHeader::Target{nullptr, 0u, 0u, 0u, 0u};
}
// ops and clear values as the caller gave them; the area, samples and views are the opening function's to add
static void take_ops(ScopeHeader& h, const mirhi_rendering_info* info) {
    h.color_load_op = info->color_load_op; h.color_store_op = info->color_store_op; h.depth_load_op = info->depth_load_op; h.depth_store_op = info->depth_store_op;
    memcpy(h.clear_color, info->clear_color, sizeof h.clear_color); h.clear_depth = info->clear_depth;
}
// Opens the scope of `p` (built in place: the frame loop records one per frame) on the images it writes (a multisampled scope: its resolve images).  Without
// a colour image the scope is depth-only: the depth image's extent is the render area's frame, and there is no colour address or format.
static mirhi_result open_scope(mirhi_cmd* cmd, RecordedPass& p, mirhi_image* color, mirhi_image* depth, mirhi_image* prim) {
    ScopeHeader& h = p.scope;
    h.depth_only = color ? 0u : 1u;
    h.color = target_of(color ? color : depth);
    if (!color) { h.color.ptr = nullptr; h.color.format = (uint32_t)MIRHI_FORMAT_UNDEFINED; }
    h.depth = target_of(depth); h.prim = target_of(prim);
    p.images.color = color; p.images.depth = depth; p.images.prim_id = prim;
    cmd->passes.push_back(std::move(p));
    cmd->in_rendering = true;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_begin_rendering(mirhi_cmd* cmd, const mirhi_rendering_info* info) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(info, "rendering_info");
    REQUIRE_NO_SCOPE(cmd);
    RecordedPass p;
    ScopeHeader& h = p.scope;
    take_ops(h, info);
    for (const mirhi_image* img : {(const mirhi_image*)info->color_image, (const mirhi_image*)info->depth_image, (const mirhi_image*)info->prim_id_image})
        if (img && img->samples != 1u)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a multisampled attachment needs a resolve target: mirhi_cmd_begin_rendering_resolve with a multisampled color_image");
    if (!info->color_image && info->depth_image) {
        // depth-only scope (MIRHI_PROGRAM_SHADOW): the depth image's extent is the render area; only SHADOW draws are recorded here
        const mirhi_image* di = info->depth_image;
        if (di->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image is not an attachment");
        if (di->format != MIRHI_FORMAT_D32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: depth attachment is not D32_SFLOAT");
        if (di->is_array) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: an image array is not an attachment: use a layer view (mirhi_image_create_layer_view)");
        if (info->prim_id_image) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: prim_id_image in a depth-only rendering scope");
        if (info->depth_store_op != MIRHI_STORE_OP_STORE)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a depth-only rendering scope must store its depth (STORE)");
        { mirhi_result ra = take_render_area(cmd, info, di->width, di->height, h.area); if (ra != MIRHI_OK) return ra; }
        return open_scope(cmd, p, nullptr, info->depth_image, nullptr);
    }
    NULL_CHECK(info->color_image, "color_image");
    const mirhi_image* ci = info->color_image;
    if (ci->is_cube || (info->depth_image && info->depth_image->is_cube) || (info->prim_id_image && info->prim_id_image->is_cube))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image is not an attachment");
    if (ci->is_array || (info->depth_image && info->depth_image->is_array))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: an image array is not an attachment: use a layer view (mirhi_image_create_layer_view)");
    if (ci->format != MIRHI_FORMAT_B8G8R8A8_SRGB && ci->format != MIRHI_FORMAT_R32G32B32A32_SFLOAT)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: color attachment has non-colour format %d", (int)ci->format);
    if (info->depth_image) {
        if (info->depth_image->format != MIRHI_FORMAT_D32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: depth attachment is not D32_SFLOAT");
        if (info->depth_image->width != ci->width || info->depth_image->height != ci->height)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: depth attachment extent does not match the colour attachment");
    }
    if (info->prim_id_image) {
        if (info->prim_id_image->format != MIRHI_FORMAT_R32_UINT || info->prim_id_image->width != ci->width || info->prim_id_image->height != ci->height)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: prim_id_image must be R32_UINT with the colour attachment's extent");
    }
    { mirhi_result ra = take_render_area(cmd, info, ci->width, ci->height, h.area); if (ra != MIRHI_OK) return ra; }
    return open_scope(cmd, p, info->color_image, info->depth_image, info->prim_id_image);
}
// A 4x multisampled scope.  What the scope WRITES are the resolve images: the recorded pass names them as its attachments (the header's targets
// and the image handles -- attachment ordering, the plan cache and fill_params then see a scope that stores colour and, with a depth resolve, depth), and samples = 4
// says that its kernels are geometry_kernel_msaa and raster_kernel_msaa.  The refusals are mirhi_scope.h's (msaa_scope_refusal).
extern "C" void mirhi_resolve_info_default(mirhi_resolve_info* r) { if (r) memset(r, 0, sizeof *r); }
extern "C" mirhi_result mirhi_cmd_begin_rendering_resolve(mirhi_cmd* cmd, const mirhi_rendering_info* info, const mirhi_resolve_info* resolve) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(info, "rendering_info");
    const bool any_resolve = resolve && (resolve->color_resolve_image || resolve->depth_resolve_image || resolve->color_resolve_mode != MIRHI_RESOLVE_NONE ||
                                         resolve->depth_resolve_mode != MIRHI_RESOLVE_NONE);
    const mirhi_image* ci = info->color_image;
    if (!ci || ci->samples == 1u) {
        if (any_resolve) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a resolve needs a multisampled color_image (mirhi_image_create_multisampled)");
        return mirhi_cmd_begin_rendering(cmd, info);
    }
    REQUIRE_NO_SCOPE(cmd);
    if (ci->dev != cmd->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the color_image belongs to another device than the command buffer");
    const mirhi_image* di = info->depth_image; const mirhi_image* pi = info->prim_id_image;
    const mirhi_image* cr = resolve ? resolve->color_resolve_image : nullptr; const mirhi_image* dr = resolve ? resolve->depth_resolve_image : nullptr;
    for (const mirhi_image* img : {cr, dr, pi})
        if (img && (img->is_cube || img->is_array)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image or an image array is not an attachment (an array: use a layer view)");
    RecordedPass p;
    ScopeHeader& h = p.scope;
    take_ops(h, info);
    bool area_partial = false;
    { mirhi_result ra = take_render_area(cmd, info, ci->width, ci->height, h.area, &area_partial); if (ra != MIRHI_OK) return ra; }
    MsaaScopeFacts f{};
    f.color_samples = ci->samples; f.color_format = (uint32_t)ci->format; f.color_w = ci->width; f.color_h = ci->height;
    f.color_load_op = info->color_load_op; f.color_store_op = info->color_store_op;
    if (di) { f.has_depth = 1u; f.depth_samples = di->samples; f.depth_format = (uint32_t)di->format; f.depth_w = di->width; f.depth_h = di->height; }
    f.depth_load_op = info->depth_load_op; f.depth_store_op = info->depth_store_op;
    if (cr) { f.has_color_resolve = 1u; f.cr_samples = cr->samples; f.cr_format = (uint32_t)cr->format; f.cr_w = cr->width; f.cr_h = cr->height; f.cr_same_device = cr->dev == ci->dev; }
    f.color_resolve_mode = resolve ? resolve->color_resolve_mode : (int32_t)MIRHI_RESOLVE_NONE;
    if (dr) { f.has_depth_resolve = 1u; f.dr_samples = dr->samples; f.dr_format = (uint32_t)dr->format; f.dr_w = dr->width; f.dr_h = dr->height; f.dr_same_device = dr->dev == ci->dev; }
    f.depth_resolve_mode = resolve ? resolve->depth_resolve_mode : (int32_t)MIRHI_RESOLVE_NONE;
    if (pi) { f.has_prim = 1u; f.prim_format = (uint32_t)pi->format; f.prim_w = pi->width; f.prim_h = pi->height; }
    if (pi && pi->samples != 1u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the prim_id_image is multisampled itself");
    if (pi && pi->dev != ci->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the prim_id_image belongs to another device");
    if (di && di->dev != ci->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the depth_image belongs to another device");
    f.area_partial = area_partial; f.split_device = cmd->dev->split_world > 1; f.fragment_stats = (cmd->dev->profiling & MIRHI_PROFILE_FRAGMENTS) != 0;
    if (const char* why = msaa_scope_refusal(f)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s", why);
    h.samples = 4u;
    h.color_store_op = MIRHI_STORE_OP_STORE; h.depth_load_op = MIRHI_LOAD_OP_CLEAR;
    h.depth_store_op = dr ? MIRHI_STORE_OP_STORE : MIRHI_STORE_OP_DONT_CARE;
    return open_scope(cmd, p, resolve->color_resolve_image, resolve->depth_resolve_image, info->prim_id_image);
}
// A multiview depth scope: ONE recorded pass -- a depth-only one whose depth target is the array's base with one layer's extent -- that carries
// the view mask and where the views' matrices are.  Its draws are recorded once, like a single-view scope's; build_plan expands them to one parameter block per
// view, submit_now sends the views as one launch per stage.  The refusals are mirhi_scope.h's (multiview_scope_refusal).
static MultiviewFacts multiview_facts(const mirhi_cmd* cmd, const mirhi_rendering_info* info, const mirhi_multiview_info* mv, bool area_partial) {
    MultiviewFacts f{};
    const mirhi_image* di = info->depth_image;
    f.has_color = info->color_image != nullptr; f.has_prim = info->prim_id_image != nullptr; f.has_depth = di != nullptr;
    if (di) { f.depth_is_array = di->is_array && !di->is_cube; f.depth_samples = di->samples; f.depth_format = (uint32_t)di->format; f.layers = di->layers; }
    f.depth_load_op = info->depth_load_op; f.depth_store_op = info->depth_store_op;
    f.view_mask = mv->view_mask; f.has_constants = mv->view_constants != nullptr; f.view_stride = mv->view_stride; f.view_offset = mv->view_offset;
    f.constants_bytes = mv->view_constants ? mv->view_constants->size : 0u;
    f.area_partial = area_partial; f.split_device = cmd->dev->split_world > 1; f.fragment_stats = (cmd->dev->profiling & MIRHI_PROFILE_FRAGMENTS) != 0;
    return f;
}
extern "C" void mirhi_multiview_info_default(mirhi_multiview_info* m) { if (m) { memset(m, 0, sizeof *m); m->view_stride = 64u; } }
extern "C" mirhi_result mirhi_cmd_begin_rendering_multiview(mirhi_cmd* cmd, const mirhi_rendering_info* info, const mirhi_multiview_info* multiview) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(info, "rendering_info"); NULL_CHECK(multiview, "multiview_info");
    REQUIRE_NO_SCOPE(cmd);
    const mirhi_image* di = info->depth_image;
    RecordedPass p;
    ScopeHeader& h = p.scope;
    take_ops(h, info);
    bool area_partial = false;
    if (di && di->is_array) { mirhi_result ra = take_render_area(cmd, info, di->width, di->height, h.area, &area_partial); if (ra != MIRHI_OK) return ra; }
    if (const char* why = multiview_scope_refusal(multiview_facts(cmd, info, multiview, area_partial))) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s", why);
    if (di->dev != cmd->dev || multiview->view_constants->dev != cmd->dev)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the depth array or the view constants belong to another device than the command buffer");
    h.view_mask = multiview->view_mask; h.view_stride = multiview->view_stride; h.view_base = multiview->view_constants->ptr + multiview->view_offset;
    return open_scope(cmd, p, nullptr, info->depth_image, nullptr);
}
extern "C" mirhi_result mirhi_cmd_end_rendering(mirhi_cmd* cmd) {
    REQUIRE_RECORDING(cmd);
    if (!cmd->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: end_rendering without begin_rendering");
    cmd->in_rendering = false;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_bind_pipeline(mirhi_cmd* cmd, mirhi_pipeline* pipeline) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(pipeline, "pipeline");
    cmd->pipeline = pipeline;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_bind_vertex_buffers(mirhi_cmd* cmd, uint32_t first_binding, uint32_t count, mirhi_buffer* const* buffers, const uint64_t* offsets) {
    REQUIRE_RECORDING(cmd);
    if (count == 0) return MIRHI_OK;
    NULL_CHECK(buffers, "buffers"); NULL_CHECK(offsets, "offsets");
    if (first_binding != 0 || count != 1) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: only vertex binding 0 exists (vertex.rs:35-41)");
    NULL_CHECK(buffers[0], "buffers[0]");
    if (offsets[0] >= buffers[0]->size || (offsets[0] & 3)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: vertex buffer offset %llu out of range or unaligned", (unsigned long long)offsets[0]);
    cmd->vb = buffers[0]; cmd->vb_offset = offsets[0];
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_bind_index_buffer(mirhi_cmd* cmd, mirhi_buffer* buffer, uint64_t offset, mirhi_index_type type) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(buffer, "buffer");
    if (type != MIRHI_INDEX_UINT16 && type != MIRHI_INDEX_UINT32) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown index type %d", (int)type);
    const uint64_t isz = type == MIRHI_INDEX_UINT16 ? 2 : 4;
    if (offset >= buffer->size || (offset % isz)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: index buffer offset %llu out of range or unaligned", (unsigned long long)offset);
    cmd->ib = buffer; cmd->ib_offset = offset; cmd->ib_type = type;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_bind_uniform(mirhi_cmd* cmd, mirhi_uniform_slot slot, mirhi_buffer* buffer, uint64_t offset, uint64_t range) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(buffer, "buffer");
    if ((int)slot < 0 || (int)slot >= MIRHI_SLOT_COUNT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown uniform slot %d", (int)slot);
    if (range == 0 || range == UINT64_MAX) range = buffer->size > offset ? buffer->size - offset : 0;   // VK_WHOLE_SIZE
    if (offset + range > buffer->size || range == 0 || (offset & 15))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: uniform range offset %llu + range %llu exceeds buffer %llu or offset not 16-byte aligned",
                    (unsigned long long)offset, (unsigned long long)range, (unsigned long long)buffer->size);
    cmd->uniforms[slot] = {buffer, offset, range};
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_bind_texture(mirhi_cmd* cmd, mirhi_texture_slot slot, mirhi_image* image) {
    REQUIRE_RECORDING(cmd);
    if ((int)slot < 0 || (int)slot >= MIRHI_TEXTURE_COUNT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown texture slot %d", (int)slot);
    REFUSE_MULTISAMPLED(image, "bound at a texture slot");
    if (image && image->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image cannot be bound at a texture slot (the IBL cubes are bound with mirhi_cmd_bind_ibl)");
    if (slot == MIRHI_TEXTURE_SHADOW_MAP) {       // t7 / s5 (model_pbr.hlsl:103-108): a depth image, sampled with the comparison sampler
        if (image && image->format != MIRHI_FORMAT_D32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the shadow map must be D32_SFLOAT");
        if (image && image->is_array)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the shadow map must be a 2-D image: bind a layer view, or the array with mirhi_cmd_bind_shadow_cascades");
        cmd->textures[slot] = image;
        return MIRHI_OK;
    }
    if (image && image->format != MIRHI_FORMAT_R8G8B8A8_UNORM && image->format != MIRHI_FORMAT_R8G8B8A8_SRGB)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: sampled images must be R8G8B8A8_UNORM or R8G8B8A8_SRGB");
    cmd->textures[slot] = image;
    return MIRHI_OK;
}
// set 2, bindings 3 and 4 of pixel/model_pbr_ibl_csm.hlsl:115-127: Texture2DArray<float> shadowMap (t10 / s8) and cbuffer ShadowData { CSMParams } (b3)
// (one body for both calls: blend_threshold is the blendThreshold of CalculateShadowCSMBlended, shadow_csm.hlsli:212-277; 0 = CalculateShadowCSM)
static mirhi_result bind_shadow_cascades(mirhi_cmd* cmd, mirhi_image* array, mirhi_buffer* params, uint64_t offset, uint64_t range, float blend_threshold) {
    REQUIRE_RECORDING(cmd);
    if (!array) { cmd->cascades = nullptr; cmd->cascade_params = {nullptr, 0, 0}; cmd->cascade_blend = 0.0f; return MIRHI_OK; }
    if (!std::isfinite(blend_threshold) || blend_threshold < 0.0f || blend_threshold > 1.0f)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a cascade blend threshold outside [0, 1] (got %g)", (double)blend_threshold);
    REFUSE_MULTISAMPLED(array, "bound as shadow cascades");
    if (array->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: shadow cascades are an image array, not a cube image");
    if (array->parent) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: shadow cascades are an image array, not a layer view");
    if (!array->is_array) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: shadow cascades are an image array (mirhi_image_create_array)");
    if (array->format != MIRHI_FORMAT_D32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the shadow cascades must be D32_SFLOAT");
    if (array->layers != 4u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the shadow cascades must have CASCADE_COUNT = 4 layers (got %u)", array->layers);
    NULL_CHECK(params, "buffer");
    if (params->usage != MIRHI_BUFFER_UNIFORM) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: CSMParams must be in a uniform buffer (usage %d)", (int)params->usage);
    if (range == 0 || range == UINT64_MAX) range = params->size > offset ? params->size - offset : 0;   // VK_WHOLE_SIZE
    if (offset + range > params->size || range == 0 || (offset & 15))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: uniform range offset %llu + range %llu exceeds buffer %llu or offset not 16-byte aligned",
                    (unsigned long long)offset, (unsigned long long)range, (unsigned long long)params->size);
    if (range < 336) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: CSMParams range %llu smaller than 336 bytes", (unsigned long long)range);
    cmd->cascades = array; cmd->cascade_params = {params, offset, range};
    cmd->cascade_blend = blend_threshold > 0.0f ? blend_threshold : 0.0f;      // (-0.0 is 0)
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_bind_shadow_cascades(mirhi_cmd* cmd, mirhi_image* array, mirhi_buffer* params, uint64_t offset, uint64_t range) {
    return bind_shadow_cascades(cmd, array, params, offset, range, 0.0f);
}
extern "C" mirhi_result mirhi_cmd_bind_shadow_cascades_blended(mirhi_cmd* cmd, mirhi_image* array, mirhi_buffer* params, uint64_t offset, uint64_t range, float blend_threshold) {
    return bind_shadow_cascades(cmd, array, params, offset, range, blend_threshold);
}
// set 3 of pixel/model_pbr_ibl.hlsl:133-155: TextureCube irradianceMap (t7 / s5), TextureCube prefilteredMap (t8 / s6), Texture2D<float4> brdfLUT (t9 / s7)
extern "C" mirhi_result mirhi_cmd_bind_ibl(mirhi_cmd* cmd, mirhi_image* irradiance, mirhi_image* prefiltered, mirhi_image* brdf_lut) {
    REQUIRE_RECORDING(cmd);
    if (!irradiance && !prefiltered && !brdf_lut) { for (auto& im : cmd->ibl) im = nullptr; return MIRHI_OK; }
    if (!irradiance || !prefiltered || !brdf_lut)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the IBL set is three images (irradiance, prefiltered, BRDF LUT): all of them, or all NULL to unbind");
    for (const mirhi_image* im : {(const mirhi_image*)irradiance, (const mirhi_image*)prefiltered, (const mirhi_image*)brdf_lut}) REFUSE_MULTISAMPLED(im, "bound in an IBL set");
    if (irradiance->dev != prefiltered->dev || irradiance->dev != brdf_lut->dev)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the IBL images belong to two devices");
    if (irradiance->dev != cmd->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the IBL images belong to another device than the command buffer");
    if (!irradiance->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the irradiance map must be a cube image (mirhi_image_create_cube)");
    if (!prefiltered->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the prefiltered map must be a cube image (mirhi_image_create_cube)");
    if (brdf_lut->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the BRDF LUT must be a 2-D image, not a cube image");
    if (brdf_lut->is_array || brdf_lut->parent) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the BRDF LUT must be a 2-D image, not an image array or a layer view");
    if (brdf_lut->format != MIRHI_FORMAT_R32G32B32A32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the BRDF LUT must be R32G32B32A32_SFLOAT");
    if (brdf_lut->width != brdf_lut->height) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the BRDF LUT must be square (got %u x %u)", brdf_lut->width, brdf_lut->height);
    cmd->ibl[0] = irradiance; cmd->ibl[1] = prefiltered; cmd->ibl[2] = brdf_lut;
    return MIRHI_OK;
}
// set 0, bindings 0 / 1 of pixel/skybox.hlsl: TextureCube environmentMap + its sampler
extern "C" mirhi_result mirhi_cmd_bind_skybox(mirhi_cmd* cmd, mirhi_image* environment) {
    REQUIRE_RECORDING(cmd);
    if (!environment) { cmd->skybox = nullptr; return MIRHI_OK; }
    REFUSE_MULTISAMPLED(environment, "bound as the skybox environment");
    if (!environment->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the skybox environment must be a cube image (mirhi_image_create_cube)");
    if (environment->format != MIRHI_FORMAT_R32G32B32A32_SFLOAT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the skybox environment must be R32G32B32A32_SFLOAT");
    if (environment->dev != cmd->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the skybox environment belongs to another device than the command buffer");
    cmd->skybox = environment;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_set_viewport(mirhi_cmd* cmd, const mirhi_viewport* vp) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(vp, "viewport");
    if (!(vp->width > 0.0f) || !(vp->height != 0.0f) || !(vp->min_depth >= 0.0f && vp->min_depth <= 1.0f) || !(vp->max_depth >= 0.0f && vp->max_depth <= 1.0f))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: viewport width must be > 0, height != 0, depth range within [0,1]");
    if (std::fabs(vp->x) + std::fabs(vp->width) > 8192.0f || std::fabs(vp->y) + std::fabs(vp->height) > 8192.0f)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: viewport exceeds the +-8192 px range supported by the guard band");
    cmd->viewport = *vp; cmd->has_viewport = true;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_set_scissor(mirhi_cmd* cmd, const mirhi_rect2d* sc) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(sc, "scissor");
    if (sc->x < 0 || sc->y < 0) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: scissor offset must be non-negative");
    cmd->scissor = *sc; cmd->has_scissor = true;
    return MIRHI_OK;
}

// The scope continues in a new segment that loads what the previous one stored (carry_out / carry_in): fragments keep their submission order
// across the cut, primitive ids continue.
static void cut_segment(mirhi_cmd* cmd) {
    RecordedPass next;
    {
        RecordedPass& prev = cmd->passes.back();
        prev.carry_out = true;
        next.scope = prev.scope;
        next.images = prev.images;
        next.scope.color_load_op = MIRHI_LOAD_OP_LOAD;
        next.carry_in = true;
        next.first_tri = next.total_tris = prev.total_tris;
    }
    cmd->passes.push_back(std::move(next));
}

// ---- what the two draw recorders (record_draw, record_sky_draw) share: each refusal at the place its recorder gives it ----
// the depth test of a pipeline as a segment's state keeps it (Vulkan: no depth write without the depth test); record_draw adds blending and discard
static DepthState depth_state_of(const mirhi_pipeline_desc& pd) {
    DepthState ds;
    ds.key_set = true;
    ds.test = pd.depth_test_enable ? 1u : 0u;
    ds.compare = ds.test ? (uint32_t)pd.depth_compare_op : (uint32_t)MIRHI_COMPARE_ALWAYS;
    ds.write = ds.test && pd.depth_write_enable ? 1u : 0u;
    return ds;
}
static mirhi_result require_dynamic_state(const mirhi_cmd* cmd) {
    return cmd->has_viewport && cmd->has_scissor ? MIRHI_OK : fail(MIRHI_ERR_PIPELINE, "Pipeline error: viewport and scissor are dynamic state and must be set before drawing (pipeline.rs:697)");
}
static mirhi_result require_color_format(const mirhi_pipeline_desc& pd, const ScopeHeader& scope) {
    if (pd.color_attachment_formats[0] == (int32_t)scope.color.format) return MIRHI_OK;
    return fail(MIRHI_ERR_PIPELINE, "Pipeline error: pipeline colour format %d does not match the attachment format %d", pd.color_attachment_formats[0], (int)scope.color.format);
}
static mirhi_result require_prim_ids(const RecordedPass& pass, uint32_t tri_count) {
    return (uint64_t)pass.total_tris + tri_count > (uint64_t)MAX_PRIM_ID ? fail(MIRHI_ERR_DEVICE, "Vulkan error: too many primitives in one rendering scope") : MIRHI_OK;
}
// The current scissor as inclusive corners, cut to the scope's render area (which lies inside the attachment: a full-extent scope's scissor is cut to the
// attachment's far edges): what a draw may cover lies inside the area, so the geometry kernel bins nothing into a tile the scope does not launch.
// record_draw computes scissor_partial AFTER this cut: every draw of a partial-area scope is scissor-partial, so every triangle that crosses the area's
// edge is a cut one and goes to the big list (correct -- the per-pixel box test is what keeps its fragments inside -- and the reason such scopes are
// kept off the triangle-parallel variants by density: ScopePlan::density_tiles).  false: the scissor is empty, nothing can be covered.
static bool draw_scissor(const mirhi_cmd* cmd, const ScopeHeader& scope, int32_t s[4]) {
    const int32_t* a = scope.area;
    const int64_t sx0 = std::max<int64_t>(cmd->scissor.x, a[0]), sy0 = std::max<int64_t>(cmd->scissor.y, a[1]);
    const int64_t sx1 = std::min<int64_t>((int64_t)cmd->scissor.x + cmd->scissor.width, (int64_t)a[0] + a[2]) - 1;
    const int64_t sy1 = std::min<int64_t>((int64_t)cmd->scissor.y + cmd->scissor.height, (int64_t)a[1] + a[3]) - 1;
    s[0] = (int32_t)sx0; s[1] = (int32_t)sy0; s[2] = (int32_t)sx1; s[3] = (int32_t)sy1;
    return sx0 <= sx1 && sy0 <= sy1;
}
// an image the segment's draws sample: ordered across lanes like an attachment (for_each_attachment)
static void note_sampled(RecordedPass& pass, mirhi_image* img) {
    if (std::find(pass.sampled.begin(), pass.sampled.end(), img) == pass.sampled.end()) pass.sampled.push_back(img);
}

// A SKYBOX draw (include/mirhi.h "SKYBOX"): always a segment of its own, set up here -- the triangle's edge functions, the three vertex values of
// LocalPos (divided on the host, in double) as an affine function of the pixel centre, scissor, depth state -- from the push constants, viewport and
// scissor of this moment.
static mirhi_result record_sky_draw(mirhi_cmd* cmd, bool indexed, uint32_t count, uint32_t instance_count, uint32_t first) {
    const mirhi_pipeline_desc& pd = cmd->pipeline->desc;
    if (indexed) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a SKYBOX pipeline draws with mirhi_cmd_draw(cmd, 3, 1, 0, 0): draw_indexed has nothing to index");
    const ScopeHeader& scope = cmd->passes.back().scope;      // (for the refusals only: the cut below moves the segments)
    if (scope.depth_only) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a SKYBOX draw in a depth-only rendering scope (pixel/skybox.hlsl writes colour)");
    if (scope.samples != 1u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a SKYBOX draw in a multisampled scope");
    if (pd.blend_enable || pd.fragment_discard_enable) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a SKYBOX draw with blending or fragment discard");
    if (count != 3u || first != 0u || instance_count > 1u)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a SKYBOX draw is vertex_count 3, first_vertex 0, instance_count 1 (got %u, %u, %u)", count, first, instance_count);
    if (!cmd->skybox) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: program %d (SKYBOX) needs an environment cube bound (mirhi_cmd_bind_skybox)", pd.fragment_program);
    mirhi_result r;
    if ((r = require_dynamic_state(cmd)) != MIRHI_OK || (r = require_color_format(pd, scope)) != MIRHI_OK) return r;
    if (instance_count == 0) return MIRHI_OK;
    if ((r = require_prim_ids(cmd->passes.back(), 1u)) != MIRHI_OK) return r;
    if (pd.depth_test_enable && pd.depth_compare_op == MIRHI_COMPARE_NEVER) { cmd->passes.back().total_tris += 1u; return MIRHI_OK; }     // draws nothing, keeps its id
    const DepthState ds = depth_state_of(pd);
    // a segment of its own, even when its depth state equals its neighbour's; a segment that holds no draw yet (nothing recorded, or only draws that
    // kept their ids and drew nothing: NEVER, an empty scissor) becomes the sky segment
    {
        const RecordedPass& back = cmd->passes.back();
        if (back.sky.on || !back.draws.empty()) cut_segment(cmd);
    }
    RecordedPass& pass = cmd->passes.back();
    pass.state = ds;
    RecordedPass::SkyDraw& k = pass.sky;
    k.on = 1u;
    k.env = cmd->skybox->ptr; k.size = cmd->skybox->width; k.levels = cmd->skybox->levels; k.seamless = cmd->skybox->cube_seamless;
    k.compare = ds.compare; k.write = ds.write; k.prim = pass.total_tris;
    const mirhi_viewport& vp = cmd->viewport;
    { float f = vp.max_depth; f = f > 0.0f ? (f < 1.0f ? f : 1.0f) : 0.0f; memcpy(&k.depth_bits, &f, 4); }
    // viewport transform and snap of the three vertices, as setup_triangle has them (clip w = 1)
    const float hw = 0.5f * vp.width, hh = 0.5f * vp.height, cx = vp.x + hw, cy = vp.y + hh;
    static const float clip[3][2] = {{-1.0f, -1.0f}, {3.0f, -1.0f}, {-1.0f, 3.0f}};      // vertex/skybox.hlsl: SV_VertexID 0, 1, 2
    int32_t X[3], Y[3];
    bool in_range = true;
    for (int i = 0; i < 3; i++) {
        const float xs = clip[i][0] * hw + cx, ys = clip[i][1] * hh + cy;
        in_range = in_range && std::fabs(xs) <= 32768.0f && std::fabs(ys) <= 32768.0f;      // (mirhi_cmd_set_viewport keeps |x| + |width| <= 8192: always)
        X[i] = (int32_t)std::rint(xs * 256.0f); Y[i] = (int32_t)std::rint(ys * 256.0f);
    }
    const int64_t S = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) - (int64_t)(X[2] - X[0]) * (int64_t)(Y[1] - Y[0]);
    const bool front = pd.front_face == 0 ? S < 0 : S > 0;                                  // the geometry kernel's winding rule (Vulkan: a = -S / 2)
    bool visible = in_range && S != 0 && pd.cull_mode != 3 && !(pd.cull_mode == 2 && !front) && !(pd.cull_mode == 1 && front);
    if (S < 0) { std::swap(X[1], X[2]); std::swap(Y[1], Y[2]); }
    for (int i = 0; i < 3; i++) {
        const int a = i, b = (i + 1) % 3;
        const int32_t dx = X[b] - X[a], dy = Y[b] - Y[a];
        const bool topleft = dy < 0 || (dy == 0 && dx > 0);
        k.a[i] = -dy; k.b[i] = dx;
        k.e0[i] = (int64_t)k.a[i] * (128 - X[a]) + (int64_t)k.b[i] * (128 - Y[a]) + (topleft ? 0 : -1);      // E_i + bias at the centre of pixel (0, 0)
    }
    if (!draw_scissor(cmd, pass.scope, k.scissor)) { visible = false; k.scissor[0] = k.scissor[1] = 0; k.scissor[2] = k.scissor[3] = -1; }
    k.visible = visible ? 1u : 0u;
    // LocalPos = (M (x, -y, 1, 1)).xyz / .w per vertex (vertex/skybox.hlsl:40-42), M = push constants [0, 64) in CameraData.viewProjection's convention
    float M[16];
    memcpy(M, cmd->push_constants, sizeof M);
    double L[3][3];
    for (int i = 0; i < 3; i++) {
        // (in double from the float32 matrix: w.w is the difference of the two far-plane terms, -9.99 + 10 for near 0.1 / far 100, and a float32 sum
        // leaves 1e-6 of it per vertex -- measured as 2e-5 of the frame against the float64 model, 1e-6 so)
        const double v[4] = {(double)clip[i][0], -(double)clip[i][1], 1.0, 1.0};
        double w[4];
        for (int r = 0; r < 4; r++) w[r] = (((double)M[r] * v[0] + (double)M[4 + r] * v[1]) + (double)M[8 + r] * v[2]) + (double)M[12 + r] * v[3];
        for (int r = 0; r < 3; r++) L[i][r] = w[r] / w[3];
    }
    // ... interpolated affinely: L(xn, yn) = L0 + (L1 - L0) (xn + 1) / 4 + (L2 - L0) (yn + 1) / 4 with xn = (x - cx) / hw, yn = (y - cy) / hh
    for (int r = 0; r < 3; r++) {
        const double dx = (L[1][r] - L[0][r]) / (4.0 * (double)hw), dy = (L[2][r] - L[0][r]) / (4.0 * (double)hh);
        k.posx[r] = (float)dx; k.posy[r] = (float)dy;
        k.pos0[r] = (float)(L[0][r] + dx * ((double)hw - (double)cx) + dy * ((double)hh - (double)cy));
    }
    note_sampled(pass, cmd->skybox);
    pass.total_tris += 1u;
    return MIRHI_OK;
}

static mirhi_result record_draw(mirhi_cmd* cmd, bool indexed, uint32_t count, uint32_t instance_count, uint32_t first, int32_t vertex_offset) {
    REQUIRE_RECORDING(cmd);
    if (!cmd->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: draw outside a rendering scope");
    if (!cmd->pipeline) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: no pipeline bound");
    const ScopeHeader& scope = cmd->passes.back().scope;      // (for the refusals only: a cut below moves the segments)
    if (scope.view_mask)      // (a multiview scope refuses every program but SHADOW in its own words, ahead of the depth-only scope's)
        if (const char* why = multiview_program_refusal(cmd->pipeline->desc.vertex_program)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s", why);
    if (cmd->pipeline->desc.vertex_program == MIRHI_PROGRAM_SKYBOX) return record_sky_draw(cmd, indexed, count, instance_count, first);
    if (!cmd->vb) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: no vertex buffer bound to binding 0");
    if (indexed && !cmd->ib) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: no index buffer bound");
    mirhi_result r;
    if ((r = require_dynamic_state(cmd)) != MIRHI_OK) return r;
    if (instance_count > 1) {
        // The path has no instance-rate input (binding 0 is per-vertex, vertex.rs:35-41,130-136; no program reads SV_InstanceID): instance i
        // rasterizes the same triangles again, behind instance i - 1 in primitive order -- recorded as that many draws of one instance.
        if (instance_count > 4096u) return fail(MIRHI_ERR_PIPELINE, "Pipeline error: unsupported: instance_count %u (at most 4096 per draw)", instance_count);
        for (uint32_t inst = 0; inst < instance_count; inst++) {
            const mirhi_result ri = record_draw(cmd, indexed, count, 1u, first, vertex_offset);
            if (ri != MIRHI_OK) return ri;
        }
        return MIRHI_OK;
    }
    const mirhi_pipeline_desc& pd = cmd->pipeline->desc;
    const bool shadow_prog = pd.vertex_program == MIRHI_PROGRAM_SHADOW;
    // (a multisampled scope refuses a SHADOW draw in its own words, ahead of the 1x scope's "needs a depth-only rendering scope")
    if (scope.samples == 4u && shadow_prog) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s", msaa_program_refusal(pd.fragment_program, false));
    if (scope.depth_only && !shadow_prog)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: only SHADOW draws may be recorded in a depth-only rendering scope (program %d)", pd.vertex_program);
    if (!scope.depth_only && shadow_prog)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: SHADOW draws need a depth-only rendering scope (color_image NULL, depth_image set)");
    if (pd.rasterization_samples != scope.samples)
        return fail(MIRHI_ERR_PIPELINE, "Pipeline error: pipeline rasterization_samples %u does not match the rendering scope's sample count %u", pd.rasterization_samples, scope.samples);
    if ((r = require_color_format(pd, scope)) != MIRHI_OK) return r;      // (a depth-only scope: format UNDEFINED)
    // depth state must be uniform within a rendering scope (DESIGN.md "Depth key")
    DepthState ds = depth_state_of(pd);
    const bool never = pd.depth_test_enable && pd.depth_compare_op == MIRHI_COMPARE_NEVER;
    const uint32_t tri_count = count / 3u;
    if (instance_count == 0 || tri_count == 0) return MIRHI_OK;
    if (never && scope.samples == 4u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s", msaa_draw_refusal(ds, pd.fragment_program, false, false));      // (a predicate state)
    if (never) { cmd->passes.back().total_tris += tri_count; return MIRHI_OK; }     // draws nothing, but its primitives keep their ids
    if (pd.blend_enable) {
        uint32_t* blend = ds.blend;
        blend[0] = 1; blend[1] = (uint32_t)pd.src_color_blend_factor; blend[2] = (uint32_t)pd.dst_color_blend_factor; blend[3] = (uint32_t)pd.color_blend_op;
        blend[4] = (uint32_t)pd.src_alpha_blend_factor; blend[5] = (uint32_t)pd.dst_alpha_blend_factor; blend[6] = (uint32_t)pd.alpha_blend_op;
        blend[7] = pd.color_write_mask & 0xFu;
    }
    ds.discard = pd.fragment_discard_enable ? 1u : 0u;
    if (scope.samples == 4u) {
        // a multisampled scope is one segment of what raster_kernel_msaa takes: everything else is refused here, never drawn differently (mirhi_scope.h)
        const RecordedPass& mp = cmd->passes.back();
        const bool pbr_prog = pd.fragment_program == MIRHI_PROGRAM_MODEL_PBR || pd.fragment_program == MIRHI_PROGRAM_MODEL_PBR_IBL;
        const bool shadowed = pbr_prog && (cmd->textures[MIRHI_TEXTURE_SHADOW_MAP] || cmd->cascades);
        if (const char* why = msaa_draw_refusal(ds, pd.fragment_program, shadowed, mp.state.key_set && !(mp.state == ds)))
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s", why);
    }
    if (!cmd->passes.back().state.key_set) cmd->passes.back().state = ds;
    else if (!(cmd->passes.back().state == ds) || cmd->passes.back().sky.on) {
        // One raster launch resolves one depth state (DESIGN.md "Depth key"): the scope continues in a new segment that
        // loads what the previous one stored -- fragments keep their submission order across the cut.  (Behind a SKYBOX draw: always.)
        cut_segment(cmd);
        cmd->passes.back().state = ds;
    }
    RecordedPass& pass = cmd->passes.back();

    DrawDesc d;
    memset(&d, 0, sizeof d);
    d.stride = pd.vertex_stride;
    d.vb = cmd->vb->ptr + cmd->vb_offset;
    const uint64_t vb_bytes = cmd->vb->size - cmd->vb_offset;
    const uint32_t vsize = shadow_prog ? 12u : (pd.vertex_program == MIRHI_PROGRAM_TRIANGLE ? 24u : 48u);
    if (!indexed) {
        const uint64_t last = (uint64_t)first + 3ull * tri_count;   // one past the last vertex read
        if ((last - 1) * d.stride + vsize > vb_bytes)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: draw reads vertices [%u, %llu) beyond the bound vertex buffer (%llu bytes)", first, (unsigned long long)last, (unsigned long long)vb_bytes);
        d.index_type = 0; d.first = first; d.vertex_offset = 0; d.ib = nullptr;
    } else {
        const uint64_t isz = cmd->ib_type == MIRHI_INDEX_UINT16 ? 2 : 4;
        const uint64_t ib_bytes = cmd->ib->size - cmd->ib_offset;
        if (((uint64_t)first + 3ull * tri_count) * isz > ib_bytes)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: draw_indexed reads indices [%u, %llu) beyond the bound index buffer", first, (unsigned long long)first + 3ull * tri_count);
        d.index_type = (uint32_t)isz; d.first = first; d.vertex_offset = vertex_offset; d.ib = cmd->ib->ptr + cmd->ib_offset;
    }
    d.tri_count = tri_count;
    d.prim_base = pass.total_tris;
    if ((r = require_prim_ids(pass, tri_count)) != MIRHI_OK) return r;
    d.program = (uint32_t)pd.fragment_program;
    d.cull_mode = (uint32_t)pd.cull_mode; d.front_face = (uint32_t)pd.front_face;
    // uniforms required by the program (model.hlsl:5-19, model_full.hlsl:27-50)
    auto uptr = [&](int slot, uint64_t need, const uint8_t** out, const char* name) -> mirhi_result {
        auto& u = cmd->uniforms[slot];
        if (!u.buf) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: program %d needs %s bound", pd.fragment_program, name);
        if (u.range < need) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s range %llu smaller than %llu bytes", name, (unsigned long long)u.range, (unsigned long long)need);
        *out = u.buf->ptr + u.offset;
        return MIRHI_OK;
    };
    if (d.program == MIRHI_PROGRAM_SHADOW) {
        // ShadowConstants (vertex/shadow.hlsl:7-11) in b0: lightSpaceMatrix @0, model @64 -- the vertex pre-pass reads the model matrix as a MODEL
        // draw's object and the light matrix in place of viewProjection
        const uint8_t* p = nullptr;
        if ((r = uptr(MIRHI_SLOT_CAMERA, 128, &p, "ShadowConstants (b0)")) != MIRHI_OK) return r;
        d.camera = (const float*)p;
        d.object = (const float*)(p + 64);
    } else if (d.program != MIRHI_PROGRAM_TRIANGLE) {
        const uint8_t* p = nullptr;
        if ((r = uptr(MIRHI_SLOT_CAMERA, 208, &p, "CameraData (b0)")) != MIRHI_OK) return r;
        d.camera = (const float*)p;
        if ((r = uptr(MIRHI_SLOT_OBJECT, 128, &p, "ObjectData (b1)")) != MIRHI_OK) return r;
        d.object = (const float*)p;
        const bool pbr = d.program == MIRHI_PROGRAM_MODEL_PBR || d.program == MIRHI_PROGRAM_MODEL_PBR_IBL;      // the Cook-Torrance programs: same slots, textures, shadow terms
        if (d.program == MIRHI_PROGRAM_MODEL_FULL || pbr) {
            if ((r = uptr(MIRHI_SLOT_LIGHTS, 48, &d.lights, "LightUBO (b2)")) != MIRHI_OK) return r;
            if ((r = uptr(MIRHI_SLOT_MATERIAL, pbr ? 80 : 32, &d.material, "MaterialData (b3)")) != MIRHI_OK) return r;
            if (cmd->uniforms[MIRHI_SLOT_POINT_LIGHTS].buf) d.point_lights = cmd->uniforms[MIRHI_SLOT_POINT_LIGHTS].buf->ptr + cmd->uniforms[MIRHI_SLOT_POINT_LIGHTS].offset;
            if (cmd->uniforms[MIRHI_SLOT_SPOT_LIGHTS].buf) d.spot_lights = cmd->uniforms[MIRHI_SLOT_SPOT_LIGHTS].buf->ptr + cmd->uniforms[MIRHI_SLOT_SPOT_LIGHTS].offset;
            for (int t = 0; t < (pbr ? 5 : 2); t++)
                if (cmd->textures[t]) {
                    const mirhi_image* ti = cmd->textures[t];
                    d.tex[t] = ti->ptr; d.tex_w[t] = ti->width; d.tex_h[t] = ti->height; d.tex_levels[t] = ti->levels;
                    if (ti->format == MIRHI_FORMAT_R8G8B8A8_SRGB) d.tex_srgb |= 1u << t;
                    if (ti->levels > 1) d.tex_any_mips = 1;
                    // sampler state (mirhi_image_set_sampler).  Anisotropy belongs to LINEAR minification with MIP_LINEAR alone; a texture without a chain whose
                    // mag and min filters differ needs lambda, that is the UV derivatives tex_any_mips switches on
                    const mirhi_sampler_desc& sp = ti->sampler;
                    if (ti->levels > 1 && sp.min_filter == MIRHI_SAMPLER_FILTER_LINEAR && sp.mip_mode == MIRHI_MIP_LINEAR) d.tex_aniso |= (ti->max_anisotropy - 1u) << (4 * t);
                    d.tex_aniso |= (uint32_t)sp.mip_mode << (TEX_MIP_MODE_SHIFT + 2 * t);
                    d.tex_sampler |= ((uint32_t)sp.address_u | (uint32_t)sp.address_v << 2 | (uint32_t)sp.mag_filter << 4 | (uint32_t)sp.min_filter << 5) << (6 * t);
                    if (sp.mag_filter != sp.min_filter) d.tex_any_mips = 1;
                }
            if (pbr && cmd->textures[MIRHI_TEXTURE_SHADOW_MAP]) {
                // CalculateShadow (model_pbr.hlsl:238-251): the map and its ShadowParams; the shadowed raster variant resolves ordered depth keys only
                const mirhi_image* sm = cmd->textures[MIRHI_TEXTURE_SHADOW_MAP];
                if ((r = uptr(MIRHI_SLOT_SHADOW_DATA, 96, &d.shadow_data, "ShadowParams (SHADOW_DATA)")) != MIRHI_OK) return r;
                if (!ordered_key_only(ds, false))
                    return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a shadow map with blending, fragment discard or a predicate depth state");
                if (cmd->cascades)
                    return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: both a shadow map (MIRHI_TEXTURE_SHADOW_MAP) and shadow cascades (mirhi_cmd_bind_shadow_cascades) are bound");
                d.shadow_map = (const float*)sm->ptr; d.shadow_w = sm->width; d.shadow_h = sm->height;
            } else if (pbr && cmd->cascades) {
                // CalculateShadowCSM (model_pbr_ibl_csm.hlsl:280-298): the array and its CSMParams.  SV_Position.z is the depth the key holds, so the
                // draw needs an ordered depth key (depth test and write with an ordering compare op)
                const mirhi_image* ca = cmd->cascades;
                if (!ordered_key_only(ds, true))
                    return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: shadow cascades with blending, fragment discard, a predicate depth state or no depth test");
                d.shadow_map = (const float*)ca->ptr; d.shadow_w = ca->width; d.shadow_h = ca->height; d.shadow_layers = ca->layers;
                d.shadow_data = cmd->cascade_params.buf->ptr + cmd->cascade_params.offset;
                d.csm_blend = cmd->cascade_blend;
            }
            if (d.program == MIRHI_PROGRAM_MODEL_PBR_IBL) {
                // set 3 (mirhi_cmd_bind_ibl).  raster_kernel_ibl resolves ordered depth keys only, like the shadowed variants
                if (!cmd->ibl[0]) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: program %d (MODEL_PBR_IBL) needs an IBL set bound (mirhi_cmd_bind_ibl)", pd.fragment_program);
                if (!ordered_key_only(ds, false))
                    return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: MODEL_PBR_IBL with blending, fragment discard or a predicate depth state");
            }
        }
    }
    // viewport (Vulkan: xf = (w/2) xd + (x + w/2)), guard-band factors, scissor
    const mirhi_viewport& vp = cmd->viewport;
    d.hw = 0.5f * vp.width; d.hh = 0.5f * vp.height;
    d.cx = vp.x + d.hw; d.cy = vp.y + d.hh;
    d.dscale = vp.max_depth - vp.min_depth; d.dmin = vp.min_depth;
    // depth bias / depth clamp: per draw, read by setup_triangle and the outcodes alone.  The raster's clamp is to [0, 1], not to the viewport's range
    if (pd.depth_clamp_enable && !(vp.min_depth == 0.0f && vp.max_depth == 1.0f))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: depth clamp with a viewport depth range other than [0, 1] (got [%g, %g])", (double)vp.min_depth, (double)vp.max_depth);
    if (pd.depth_bias_enable) {
        const mirhi_depth_bias& b = cmd->pipeline->bias;
        d.bias_constant = b.constant_factor; d.bias_clamp = b.clamp; d.bias_slope = b.slope_factor;
        // (factors of zero add nothing: the draw is the unbiased one, bit for bit, and takes its path)
        if (b.constant_factor != 0.0f || b.slope_factor != 0.0f) d.depth_flags |= DEPTH_FLAG_BIAS;
    }
    if (pd.depth_clamp_enable) d.depth_flags |= DEPTH_FLAG_CLAMP;
    d.gx = (GUARD_PX - std::fabs(d.cx)) / d.hw;
    d.gy = (GUARD_PX - std::fabs(d.cy)) / d.hh;
    int32_t sc[4];
    if (!draw_scissor(cmd, pass.scope, sc)) return MIRHI_OK;    // empty scissor: nothing can be covered
    d.sx0 = sc[0]; d.sy0 = sc[1]; d.sx1 = sc[2]; d.sy1 = sc[3];
    d.scissor_partial = (sc[0] > 0 || sc[1] > 0 || sc[2] < (int32_t)pass.scope.color.width - 1 || sc[3] < (int32_t)pass.scope.color.height - 1) ? 1u : 0u;
    if (d.program == MIRHI_PROGRAM_MODEL_PBR_IBL) {
        // the set is per scope (PassParams): every MODEL_PBR_IBL draw of the scope, in all its segments, is recorded under the same three images
        ScopeHeader::IblSet set{};
        set.irradiance = cmd->ibl[0]->ptr; set.prefiltered = cmd->ibl[1]->ptr; set.lut = cmd->ibl[2]->ptr;
        set.irr_size = cmd->ibl[0]->width; set.pre_size = cmd->ibl[1]->width; set.pre_levels = cmd->ibl[1]->levels; set.lut_size = cmd->ibl[2]->width;
        set.seamless = (cmd->ibl[0]->cube_seamless ? 1u : 0u) | (cmd->ibl[1]->cube_seamless ? 2u : 0u);      // (latched here; the LUT is 2-D and has no such state)
        if (pass.scope.ibl.irradiance && !(pass.scope.ibl == set))
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: MODEL_PBR_IBL draws recorded under two different IBL sets in one rendering scope");
        pass.scope.ibl = set;
        for (mirhi_image* im : cmd->ibl) note_sampled(pass, im);
    }
    if (d.shadow_map) {
        // one raster variant per scope: CalculateShadow (raster_kernel_shadow) or CalculateShadowCSM (raster_kernel_csm; raster_kernel_csm_blend when some
        // cascaded draw blends: blended and unblended cascaded draws share a scope, classify_scope)
        for (const DrawDesc& o : pass.draws)
            if (o.shadow_map && (o.shadow_layers != 0u) != (d.shadow_layers != 0u))
                return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: draws with a single shadow map and draws with shadow cascades in one rendering scope");
        note_sampled(pass, d.shadow_layers ? cmd->cascades : cmd->textures[MIRHI_TEXTURE_SHADOW_MAP]);
    }
    pass.draws.push_back(d);
    pass.draw_vb_bytes.push_back(vb_bytes);
    pass.total_tris += tri_count;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_draw(mirhi_cmd* cmd, uint32_t vertex_count, uint32_t instance_count, uint32_t first_vertex, uint32_t first_instance) {
    (void)first_instance;
    return record_draw(cmd, false, vertex_count, instance_count, first_vertex, 0);
}
extern "C" mirhi_result mirhi_cmd_draw_indexed(mirhi_cmd* cmd, uint32_t index_count, uint32_t instance_count, uint32_t first_index, int32_t vertex_offset, uint32_t first_instance) {
    (void)first_instance;
    return record_draw(cmd, true, index_count, instance_count, first_index, vertex_offset);
}

// draw_indirect / draw_indexed_indirect (command.rs:630-661): the arguments are fetched from the device buffer now, at record time
static mirhi_result record_indirect(mirhi_cmd* cmd, bool indexed, mirhi_buffer* buffer, uint64_t offset, uint32_t draw_count, uint32_t stride) {
    REQUIRE_RECORDING(cmd); NULL_CHECK(buffer, "buffer");
    if (buffer->dev != cmd->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: indirect buffer belongs to another device");
    if (cmd->pipeline && cmd->pipeline->desc.vertex_program == MIRHI_PROGRAM_SKYBOX)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a SKYBOX pipeline draws with mirhi_cmd_draw(cmd, 3, 1, 0, 0): no indirect draws");
    const uint32_t words = indexed ? 5u : 4u;
    if (draw_count == 0) return MIRHI_OK;
    if ((offset & 3u) || (draw_count > 1 && (stride < words * 4u || (stride & 3u))))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: indirect offset %llu / stride %u must be multiples of 4 (stride >= %u)", (unsigned long long)offset, stride, words * 4u);
    const uint64_t step = draw_count > 1 ? stride : words * 4u;
    const uint64_t span = (uint64_t)(draw_count - 1) * step + words * 4u;
    if (offset + span > buffer->size || offset + span < offset)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: indirect draws read [%llu, %llu) beyond the buffer (%llu bytes)", (unsigned long long)offset,
                    (unsigned long long)(offset + span), (unsigned long long)buffer->size);
    std::vector<uint8_t> host(span);
    { mirhi_result r0 = sync_all_lanes(cmd->dev); if (r0 != MIRHI_OK) return r0; }
    HIP_TRY(hipMemcpyAsync(host.data(), buffer->ptr + offset, span, hipMemcpyDeviceToHost, cmd->dev->stream));
    HIP_TRY(hipStreamSynchronize(cmd->dev->stream));
    for (uint32_t i = 0; i < draw_count; i++) {
        uint32_t a[5] = {0, 0, 0, 0, 0};
        memcpy(a, host.data() + (size_t)i * step, words * 4u);
        const mirhi_result r = indexed ? record_draw(cmd, true, a[0], a[1], a[2], (int32_t)a[3]) : record_draw(cmd, false, a[0], a[1], a[2], 0);
        if (r != MIRHI_OK) return r;
    }
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_draw_indirect(mirhi_cmd* cmd, mirhi_buffer* buffer, uint64_t offset, uint32_t draw_count, uint32_t stride) {
    return record_indirect(cmd, false, buffer, offset, draw_count, stride);
}
extern "C" mirhi_result mirhi_cmd_draw_indexed_indirect(mirhi_cmd* cmd, mirhi_buffer* buffer, uint64_t offset, uint32_t draw_count, uint32_t stride) {
    return record_indirect(cmd, true, buffer, offset, draw_count, stride);
}
extern "C" mirhi_result mirhi_cmd_push_constants(mirhi_cmd* cmd, uint32_t stage_flags, uint32_t offset, const void* data, uint32_t len) {
    REQUIRE_RECORDING(cmd);
    (void)stage_flags;
    if (len == 0) return MIRHI_OK;
    NULL_CHECK(data, "data");
    if ((offset & 3u) || (len & 3u) || (uint64_t)offset + len > sizeof cmd->push_constants)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: push constants offset %u + size %u must be multiples of 4 within %zu bytes", offset, len, sizeof cmd->push_constants);
    memcpy(cmd->push_constants + offset, data, len);
    return MIRHI_OK;
}

// ---- transfer commands (include/mirhi.h "Transfer commands"; command.rs:844-1019) -------------------------------------------------------
// A transfer command is an entry of the recording of its own: a RecordedPass with `xfer` set and no attachments, draws, bins or vertex job.  Its
// regions are resolved here, at record time, into what the kernels of mirhi_transfer.hip.h take (XferRegion); everything that can be refused is.
struct XferLevel { uint8_t* base; uint32_t w, h, bpp; mirhi_format format; };
// one 2-D level of `img` as a transfer's source or destination: 2-D images, layer views, the levels of an image with a chain
static mirhi_result xfer_level(const mirhi_cmd* cmd, const mirhi_image* img, uint32_t level, const char* what, XferLevel* out) {
    if (!img) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s is null", what);
    if (img->dev != cmd->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the %s belongs to another device than the command buffer", what);
    REFUSE_MULTISAMPLED(img, "a transfer's source or destination");
    if (img->is_cube) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: a cube image is not a transfer's %s", what);
    if (img->is_array) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: an image array is not a transfer's %s: use a layer view (mirhi_image_create_layer_view)", what);
    if (level >= img->levels) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: mip level %u of the %s out of range (the image has %u)", level, what, img->levels);
    const uint32_t bpp = format_bpp(img->format);
    uint32_t w = img->width, h = img->height;
    size_t texels = 0;
    for (uint32_t l = 0; l < level; l++) { texels += (size_t)w * h; w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1; }
    *out = XferLevel{img->ptr + texels * bpp, w, h, bpp, img->format};
    return MIRHI_OK;
}
static mirhi_result xfer_buffer(const mirhi_cmd* cmd, const mirhi_buffer* buf, const char* what) {
    if (!buf) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s is null", what);
    if (buf->dev != cmd->dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the %s belongs to another device than the command buffer", what);
    return MIRHI_OK;
}
static mirhi_result xfer_begin(mirhi_cmd* cmd, const char* name, uint32_t region_count, const void* regions) {
    REQUIRE_RECORDING(cmd);
    if (cmd->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: %s inside an active rendering scope (transfer commands are recorded outside)", name);
    if (region_count == 0u || region_count > XFER_MAX_REGIONS)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region_count %u must be in [1, %u]", name, region_count, XFER_MAX_REGIONS);
    NULL_CHECK(regions, "regions");
    return MIRHI_OK;
}
// a rectangle of a level: offset >= 0, extent > 0, offset + extent inside
static mirhi_result xfer_rect(const char* name, uint32_t i, const char* what, const XferLevel& L, const int32_t off[2], const uint32_t ext[2]) {
    if (ext[0] == 0u || ext[1] == 0u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u has a zero extent", name, i);
    if (off[0] < 0 || off[1] < 0 || (uint64_t)off[0] + ext[0] > L.w || (uint64_t)off[1] + ext[1] > L.h)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u is outside its %s (offset %d, %d extent %u x %u, level %u x %u)", name, i, what, off[0], off[1], ext[0], ext[1], L.w, L.h);
    return MIRHI_OK;
}
// the copy of one rectangle; rows that are whole and tight on both sides become one run
static XferRegion xfer_copy_region(const uint8_t* src, uint64_t src_pitch, uint8_t* dst, uint64_t dst_pitch, uint64_t row_bytes, uint32_t rows) {
    XferRegion g;
    memset(&g, 0, sizeof g);
    if (rows > 1u && src_pitch == row_bytes && dst_pitch == row_bytes) { row_bytes *= rows; rows = 1u; }
    g.src = src; g.dst = dst; g.src_pitch = src_pitch; g.dst_pitch = dst_pitch; g.row_bytes = row_bytes; g.rows = rows;
    const uint64_t apart = (uint64_t)(uintptr_t)src ^ (uint64_t)(uintptr_t)dst, pitches = rows > 1u ? (src_pitch ^ dst_pitch) : 0u;
    g.unit = ((apart | pitches) & 15u) == 0u ? 16u : (((apart | pitches) & 3u) == 0u ? 4u : 1u);      // (x ^ y has the low bits of x - y)
    const uint64_t accesses = row_bytes / g.unit;
    g.chunks = (uint32_t)std::max<uint64_t>(1u, (accesses + 1023u) / 1024u);
    return g;
}
// the entry itself: numbers the regions' work units through, notes the images for ordering across lanes and the buffers' spans for mirhi_buffer_write
static mirhi_result xfer_push(mirhi_cmd* cmd, const char* name, uint32_t kind, std::vector<XferRegion>& regions, const std::vector<uint64_t>& units,
                              mirhi_image* src_img, mirhi_image* dst_img, const mirhi_buffer* src_buf, const mirhi_buffer* dst_buf,
                              uint32_t src_format, uint32_t dst_format, const float color[4]) {
    uint64_t total = 0;
    for (size_t i = 0; i < regions.size(); i++) { regions[i].first = (uint32_t)total; total += units[i]; if (total >= (1ull << 31)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: too much work for one command", name); }
    RecordedPass p;
    RecordedPass::Transfer& t = p.xfer;
    t.kind = kind; t.count = (uint32_t)regions.size(); t.src_format = src_format; t.dst_format = dst_format;
    if (color) memcpy(t.color, color, sizeof t.color);
    t.groups = (uint32_t)total;
    t.grid = (kind == XFER_COPY || kind == XFER_FILL) ? (uint32_t)std::min<uint64_t>(total, XFER_MAX_GROUPS) : (uint32_t)total;
    if (src_buf) { t.span[0] = src_buf->ptr; t.span[1] = src_buf->ptr + src_buf->size; }
    if (dst_buf) { t.span[2] = dst_buf->ptr; t.span[3] = dst_buf->ptr + dst_buf->size; }
    p.xfer_regions = std::move(regions);
    // a destination image is ordered like an attachment, a source image like a sampled shadow map (for_each_attachment; a layer view stands for its array)
    if (src_img) p.sampled.push_back(src_img);
    if (dst_img && dst_img != src_img) p.sampled.push_back(dst_img);
    cmd->passes.push_back(std::move(p));
    return MIRHI_OK;
}
static bool xfer_ranges_overlap(const uint8_t* a, uint64_t an, const uint8_t* b, uint64_t bn) { return a < b + bn && b < a + an; }

extern "C" mirhi_result mirhi_cmd_copy_buffer(mirhi_cmd* cmd, mirhi_buffer* src, mirhi_buffer* dst, uint32_t region_count, const mirhi_buffer_copy* regions) {
    static const char* const name = "copy_buffer";
    mirhi_result r = xfer_begin(cmd, name, region_count, regions);
    if (r != MIRHI_OK || (r = xfer_buffer(cmd, src, "source buffer")) != MIRHI_OK || (r = xfer_buffer(cmd, dst, "destination buffer")) != MIRHI_OK) return r;
    std::vector<XferRegion> out; std::vector<uint64_t> units;
    for (uint32_t i = 0; i < region_count; i++) {
        const mirhi_buffer_copy& c = regions[i];
        if (c.size == 0u) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u has size 0", name, i);
        if (c.src_offset + c.size < c.src_offset || c.dst_offset + c.size < c.dst_offset)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u: offset + size overflows", name, i);
        if (c.src_offset + c.size > src->size || c.dst_offset + c.size > dst->size)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u is outside its buffer (source %llu + %llu of %llu, destination %llu + %llu of %llu)", name, i,
                        (unsigned long long)c.src_offset, (unsigned long long)c.size, (unsigned long long)src->size, (unsigned long long)c.dst_offset, (unsigned long long)c.size, (unsigned long long)dst->size);
        out.push_back(xfer_copy_region(src->ptr + c.src_offset, 0u, dst->ptr + c.dst_offset, 0u, c.size, 1u));
        units.push_back(out.back().chunks);
    }
    // (by address: two handles may wrap one piece of memory)
    for (uint32_t i = 0; i < region_count; i++)
        for (uint32_t j = 0; j < region_count; j++)
            if (xfer_ranges_overlap(out[i].src, out[i].row_bytes, out[j].dst, out[j].row_bytes))
                return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: the source range of region %u and the destination range of region %u are overlapping", name, i, j);
    return xfer_push(cmd, name, XFER_COPY, out, units, nullptr, nullptr, src, dst, 0u, 0u, nullptr);
}

static mirhi_result xfer_buffer_image(mirhi_cmd* cmd, const char* name, mirhi_buffer* buf, mirhi_image* img, bool to_image, uint32_t region_count, const mirhi_buffer_image_copy* regions) {
    mirhi_result r = xfer_begin(cmd, name, region_count, regions);
    if (r != MIRHI_OK || (r = xfer_buffer(cmd, buf, to_image ? "source buffer" : "destination buffer")) != MIRHI_OK) return r;
    std::vector<XferRegion> out; std::vector<uint64_t> units;
    for (uint32_t i = 0; i < region_count; i++) {
        const mirhi_buffer_image_copy& c = regions[i];
        XferLevel L;
        if ((r = xfer_level(cmd, img, c.mip_level, to_image ? "destination image" : "source image", &L)) != MIRHI_OK) return r;
        if ((r = xfer_rect(name, i, "image", L, c.image_offset, c.image_extent)) != MIRHI_OK) return r;
        if ((c.buffer_row_length && c.buffer_row_length < c.image_extent[0]) || (c.buffer_image_height && c.buffer_image_height < c.image_extent[1]))
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u: buffer_row_length %u / buffer_image_height %u must be 0 (tightly packed) or at least the extent %u x %u", name, i,
                        c.buffer_row_length, c.buffer_image_height, c.image_extent[0], c.image_extent[1]);
        if (c.buffer_offset % L.bpp) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u: buffer_offset %llu is not a multiple of the texel size %u", name, i, (unsigned long long)c.buffer_offset, L.bpp);
        const uint64_t pitch = (uint64_t)(c.buffer_row_length ? c.buffer_row_length : c.image_extent[0]) * L.bpp, row_bytes = (uint64_t)c.image_extent[0] * L.bpp;
        const uint64_t need = pitch * (c.image_extent[1] - 1u) + row_bytes;
        if (c.buffer_offset + need < c.buffer_offset) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u: buffer_offset + size overflows", name, i);
        if (c.buffer_offset + need > buf->size)
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u is outside its buffer (offset %llu + %llu bytes of %llu)", name, i, (unsigned long long)c.buffer_offset, (unsigned long long)need, (unsigned long long)buf->size);
        uint8_t* const ip = L.base + ((size_t)c.image_offset[1] * L.w + (size_t)c.image_offset[0]) * L.bpp;
        uint8_t* const bp = buf->ptr + c.buffer_offset;
        const uint64_t ipitch = (uint64_t)L.w * L.bpp;
        out.push_back(to_image ? xfer_copy_region(bp, pitch, ip, ipitch, row_bytes, c.image_extent[1]) : xfer_copy_region(ip, ipitch, bp, pitch, row_bytes, c.image_extent[1]));
        units.push_back((uint64_t)out.back().rows * out.back().chunks);
    }
    return xfer_push(cmd, name, XFER_COPY, out, units, to_image ? nullptr : img, to_image ? img : nullptr, to_image ? buf : nullptr, to_image ? nullptr : buf, 0u, 0u, nullptr);
}
extern "C" mirhi_result mirhi_cmd_copy_buffer_to_image(mirhi_cmd* cmd, mirhi_buffer* src_buffer, mirhi_image* dst_image, uint32_t region_count, const mirhi_buffer_image_copy* regions) {
    return xfer_buffer_image(cmd, "copy_buffer_to_image", src_buffer, dst_image, true, region_count, regions);
}
extern "C" mirhi_result mirhi_cmd_copy_image_to_buffer(mirhi_cmd* cmd, mirhi_image* src_image, mirhi_buffer* dst_buffer, uint32_t region_count, const mirhi_buffer_image_copy* regions) {
    return xfer_buffer_image(cmd, "copy_image_to_buffer", dst_buffer, src_image, false, region_count, regions);
}

extern "C" mirhi_result mirhi_cmd_copy_image(mirhi_cmd* cmd, mirhi_image* src_image, mirhi_image* dst_image, uint32_t region_count, const mirhi_image_copy* regions) {
    static const char* const name = "copy_image";
    mirhi_result r = xfer_begin(cmd, name, region_count, regions);
    if (r != MIRHI_OK) return r;
    std::vector<XferRegion> out; std::vector<uint64_t> units;
    struct Rect { const uint8_t* base; int32_t x, y; uint32_t w, h; };
    std::vector<Rect> srcs, dsts;
    for (uint32_t i = 0; i < region_count; i++) {
        const mirhi_image_copy& c = regions[i];
        XferLevel S, D;
        if ((r = xfer_level(cmd, src_image, c.src_mip_level, "source image", &S)) != MIRHI_OK || (r = xfer_level(cmd, dst_image, c.dst_mip_level, "destination image", &D)) != MIRHI_OK) return r;
        if (S.bpp != D.bpp || (S.format == MIRHI_FORMAT_D32_SFLOAT) != (D.format == MIRHI_FORMAT_D32_SFLOAT))
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: formats %d and %d are not copy-compatible (equal texel size, both colour or both D32_SFLOAT)", name, (int)S.format, (int)D.format);
        if ((r = xfer_rect(name, i, "source image", S, c.src_offset, c.extent)) != MIRHI_OK || (r = xfer_rect(name, i, "destination image", D, c.dst_offset, c.extent)) != MIRHI_OK) return r;
        srcs.push_back(Rect{S.base, c.src_offset[0], c.src_offset[1], c.extent[0], c.extent[1]});
        dsts.push_back(Rect{D.base, c.dst_offset[0], c.dst_offset[1], c.extent[0], c.extent[1]});
        out.push_back(xfer_copy_region(S.base + ((size_t)c.src_offset[1] * S.w + (size_t)c.src_offset[0]) * S.bpp, (uint64_t)S.w * S.bpp,
                                       D.base + ((size_t)c.dst_offset[1] * D.w + (size_t)c.dst_offset[0]) * D.bpp, (uint64_t)D.w * D.bpp, (uint64_t)c.extent[0] * S.bpp, c.extent[1]));
        units.push_back((uint64_t)out.back().rows * out.back().chunks);
    }
    for (const Rect& a : srcs)
        for (const Rect& b : dsts)
            if (a.base == b.base && a.x < b.x + (int32_t)b.w && b.x < a.x + (int32_t)a.w && a.y < b.y + (int32_t)b.h && b.y < a.y + (int32_t)a.h)
                return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: source and destination regions of one image level are overlapping", name);
    return xfer_push(cmd, name, XFER_COPY, out, units, src_image, dst_image, nullptr, nullptr, 0u, 0u, nullptr);
}

static bool xfer_blit_format(mirhi_format f) {
    return f == MIRHI_FORMAT_B8G8R8A8_SRGB || f == MIRHI_FORMAT_R8G8B8A8_UNORM || f == MIRHI_FORMAT_R8G8B8A8_SRGB || f == MIRHI_FORMAT_R32G32B32A32_SFLOAT;
}
extern "C" mirhi_result mirhi_cmd_blit_image(mirhi_cmd* cmd, mirhi_image* src_image, mirhi_image* dst_image, uint32_t region_count, const mirhi_image_blit* regions, mirhi_filter filter) {
    static const char* const name = "blit_image";
    mirhi_result r = xfer_begin(cmd, name, region_count, regions);
    if (r != MIRHI_OK) return r;
    if (filter != MIRHI_FILTER_NEAREST && filter != MIRHI_FILTER_LINEAR) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: unknown filter %d", name, (int)filter);
    std::vector<XferRegion> out; std::vector<uint64_t> units;
    uint32_t sf = 0, df = 0;
    for (uint32_t i = 0; i < region_count; i++) {
        const mirhi_image_blit& c = regions[i];
        XferLevel S, D;
        if ((r = xfer_level(cmd, src_image, c.src_mip_level, "source image", &S)) != MIRHI_OK || (r = xfer_level(cmd, dst_image, c.dst_mip_level, "destination image", &D)) != MIRHI_OK) return r;
        if (!xfer_blit_format(S.format) || !xfer_blit_format(D.format))
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: unsupported: formats %d -> %d (B8G8R8A8_SRGB, R8G8B8A8_UNORM, R8G8B8A8_SRGB and R32G32B32A32_SFLOAT are blitted)", name, (int)S.format, (int)D.format);
        if (src_image == dst_image || (src_image->parent && src_image->parent == dst_image->parent))
            return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: the source image must differ from the destination image", name);
        sf = (uint32_t)S.format; df = (uint32_t)D.format;
        for (int a = 0; a < 2; a++) {
            const int32_t smax = (int32_t)(a ? S.h : S.w), dmax = (int32_t)(a ? D.h : D.w);
            for (int e = 0; e < 2; e++)
                if (c.src_offsets[e][a] < 0 || c.src_offsets[e][a] > smax || c.dst_offsets[e][a] < 0 || c.dst_offsets[e][a] > dmax)
                    return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u is outside its image (source level %u x %u, destination level %u x %u)", name, i, S.w, S.h, D.w, D.h);
            if (c.src_offsets[0][a] == c.src_offsets[1][a] || c.dst_offsets[0][a] == c.dst_offsets[1][a])
                return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u has zero area", name, i);
        }
        XferRegion g;
        memset(&g, 0, sizeof g);
        g.src = S.base; g.dst = D.base; g.src_w = S.w; g.src_h = S.h; g.dst_w = D.w;
        int32_t* const lo[2] = {&g.dx0, &g.dy0}; int32_t* const hi[2] = {&g.dx1, &g.dy1};
        int32_t* const s0[2] = {&g.sx0, &g.sy0}; int32_t* const n0[2] = {&g.xn0, &g.yn0}; int32_t* const ns[2] = {&g.xns, &g.yns}; int32_t* const dn[2] = {&g.xd, &g.yd};
        for (int a = 0; a < 2; a++) {
            // u = (i + 1/2 - d0) (s1 - s0) / (d1 - d0) + s0  =  s0 + sgn (2 (i - d0) + 1) (s1 - s0) / (2 |d1 - d0|);  LINEAR samples at u - 1/2
            const int64_t ds = (int64_t)c.src_offsets[1][a] - c.src_offsets[0][a], dd = (int64_t)c.dst_offsets[1][a] - c.dst_offsets[0][a];
            const int64_t sgn = dd > 0 ? 1 : -1, mag = dd > 0 ? dd : -dd;
            *lo[a] = std::min(c.dst_offsets[0][a], c.dst_offsets[1][a]); *hi[a] = std::max(c.dst_offsets[0][a], c.dst_offsets[1][a]);
            const int64_t first = sgn * (2 * ((int64_t)*lo[a] - c.dst_offsets[0][a]) + 1) * ds - (filter == MIRHI_FILTER_LINEAR ? mag : 0), step = sgn * 2 * ds;
            const int64_t reach = std::llabs(first) + std::llabs(step) * (mag + 64);      // (what a lane of an edge tile may form)
            if (reach >= (1ll << 31)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: region %u: offsets overflow", name, i);
            *s0[a] = c.src_offsets[0][a]; *n0[a] = (int32_t)first; *ns[a] = (int32_t)step; *dn[a] = (int32_t)(2 * mag);
        }
        g.tiles_x = (uint32_t)(((g.dx1 - 1) >> 5) - (g.dx0 >> 5) + 1);
        const uint32_t tiles_y = (uint32_t)(((g.dy1 - 1) >> 5) - (g.dy0 >> 5) + 1);
        out.push_back(g);
        units.push_back((uint64_t)g.tiles_x * tiles_y);
    }
    return xfer_push(cmd, name, filter == MIRHI_FILTER_LINEAR ? XFER_BLIT_LINEAR : XFER_BLIT_NEAREST, out, units, src_image, dst_image, nullptr, nullptr, sf, df, nullptr);
}

// a clear: one range -- the whole image with every level of its chain, or the one layer a view stands for
static mirhi_result xfer_clear(mirhi_cmd* cmd, const char* name, mirhi_image* image, const float color[4]) {
    XferLevel L;
    mirhi_result r = xfer_level(cmd, image, 0u, "image", &L);
    if (r != MIRHI_OK) return r;
    size_t texels = 0;
    uint32_t w = image->width, h = image->height;
    for (uint32_t l = 0; l < image->levels; l++) { texels += (size_t)w * h; w = w > 1 ? w >> 1 : 1; h = h > 1 ? h >> 1 : 1; }
    XferRegion g;
    memset(&g, 0, sizeof g);
    g.dst = L.base; g.row_bytes = (uint64_t)texels * L.bpp; g.rows = 1u; g.unit = 16u;
    g.chunks = (uint32_t)std::max<uint64_t>(1u, (g.row_bytes / 16u + 1023u) / 1024u);
    std::vector<XferRegion> out{g}; std::vector<uint64_t> units{g.chunks};
    return xfer_push(cmd, name, XFER_FILL, out, units, nullptr, image, nullptr, nullptr, 0u, (uint32_t)L.format, color);
}
extern "C" mirhi_result mirhi_cmd_clear_color_image(mirhi_cmd* cmd, mirhi_image* image, const float color[4]) {
    static const char* const name = "clear_color_image";
    REQUIRE_RECORDING(cmd); NULL_CHECK(color, "color");
    if (cmd->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: %s inside an active rendering scope (transfer commands are recorded outside)", name);
    if (image && !image->is_cube && !image->is_array && !xfer_blit_format(image->format))
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: unsupported: format %d (B8G8R8A8_SRGB, R8G8B8A8_UNORM, R8G8B8A8_SRGB and R32G32B32A32_SFLOAT are cleared)", name, (int)image->format);
    return xfer_clear(cmd, name, image, color);
}
extern "C" mirhi_result mirhi_cmd_clear_depth_stencil_image(mirhi_cmd* cmd, mirhi_image* image, float depth) {
    static const char* const name = "clear_depth_stencil_image";
    REQUIRE_RECORDING(cmd);
    if (cmd->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: %s inside an active rendering scope (transfer commands are recorded outside)", name);
    if (image && !image->is_cube && !image->is_array && image->format != MIRHI_FORMAT_D32_SFLOAT)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: %s: format %d is not D32_SFLOAT", name, (int)image->format);
    const float value[4] = {depth, 0.0f, 0.0f, 0.0f};
    return xfer_clear(cmd, name, image, value);
}

// ---- end(): size the workspace and build the launch plan ------------------------------------------
template <typename T>
static mirhi_result grow(T** ptr, size_t* have, size_t want_bytes) {
    if (*have >= want_bytes && *ptr) return MIRHI_OK;
    if (*ptr) { (void)hipFree(*ptr); *ptr = nullptr; *have = 0; }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want_bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc(%zu) for rasterizer workspace: %s", want_bytes, hipGetErrorString(e)); }
    *ptr = (T*)p; *have = want_bytes;
    return MIRHI_OK;
}

// Sizes the workspace of a recorded command buffer and builds its launch plan.  Runs at end() -- unless the recording is the one the
// current plan was built from -- and again in front of a submit when an earlier submission exhausted the bin pool
// (Workspace::grow_pool) or showed a spread-out mesh (Workspace::replan).
static mirhi_result build_plan(mirhi_cmd* cmd, bool in_submit = false);
static mirhi_result pblock_commit(Workspace& w, hipStream_t stream);

// Two recordings describe the same frame shape: the same scopes (ScopeHeader: attachments as resolved, load / store ops, clear values, area, samples,
// views, IBL set) and, segment by segment, the same depth / blend state and, byte for byte, the same draw descriptors (resolved device pointers,
// counts, viewport, scissor, state).  Buffer CONTENTS are not part of it: the plan holds pointers, and a frame loop that rewrites its uniform buffer
// between frames records the same shape every time.
// any_color_address: the colour targets may sit at other addresses (same extent and format) -- the recording of a frame loop that cycles N + 1 swapchain images
// through N command buffers (swapchain.rs:228-236, renderer.rs:377-390): everything the plan holds but PassParams::color is the same then
static bool same_scope(const ScopeHeader& x, const ScopeHeader& y, bool any_color_address) {
    if (!any_color_address) return x == y;
    ScopeHeader a = x, b = y;      // the address replaced by "is set" on both sides
    a.color.ptr = reinterpret_cast<const uint8_t*>((uintptr_t)(x.color.ptr != nullptr)); b.color.ptr = reinterpret_cast<const uint8_t*>((uintptr_t)(y.color.ptr != nullptr));
    return a == b;
}
static bool same_recording(const std::vector<RecordedPass>& a, const std::vector<RecordedPass>& b, bool any_color_address = false) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        const RecordedPass& x = a[i]; const RecordedPass& y = b[i];
        if (!same_scope(x.scope, y.scope, any_color_address)) return false;
        if (x.total_tris != y.total_tris || x.first_tri != y.first_tri || !(x.state == y.state) || x.carry_in != y.carry_in || x.carry_out != y.carry_out) return false;
        if (x.sampled != y.sampled || !(x.sky == y.sky)) return false;
        if (!(x.xfer == y.xfer) || x.xfer_regions.size() != y.xfer_regions.size() ||
            (!x.xfer_regions.empty() && memcmp(x.xfer_regions.data(), y.xfer_regions.data(), x.xfer_regions.size() * sizeof(XferRegion)) != 0)) return false;
        if (x.draws.size() != y.draws.size() || x.draw_vb_bytes != y.draw_vb_bytes) return false;
        if (!x.draws.empty() && memcmp(x.draws.data(), y.draws.data(), x.draws.size() * sizeof(DrawDesc)) != 0) return false;
    }
    return true;
}

// The workspace of a command buffer that may still be executing must not be touched: Vulkan forbids re-recording a pending command
// buffer, this build waits for it.  A frame loop that waits on its in-flight fence first (renderer.rs:371-374) never waits here.
static mirhi_result settle_pending(mirhi_cmd* cmd, bool in_submit) {
    // (submit thread on: not before its queued submissions have been issued -- unless this IS the submit thread, re-planning the job it holds)
    while (!in_submit && cmd->queued.load(std::memory_order_acquire) > 0) cpu_relax();
    if (!cmd->pending) return MIRHI_OK;
    mirhi_device* dev = cmd->dev;
    if (cmd->last_native && !drain_native(dev, cmd->last_native)) return device_lost(dev);
    bool live = false;
    for (hipStream_t st : dev->lanes) live |= st == cmd->last_stream;
    if (live) HIP_TRY(hipStreamSynchronize(cmd->last_stream));
    cmd_finished(cmd);
    return MIRHI_OK;
}

static bool recording_reads(const std::vector<RecordedPass>& passes, const uint8_t* lo, const uint8_t* hi) {
    auto in = [&](const void* q) { return q && (const uint8_t*)q >= lo && (const uint8_t*)q < hi; };
    for (const RecordedPass& pass : passes) {
        for (const DrawDesc& d : pass.draws) {
            if (in(d.vb) || in(d.ib) || in(d.camera) || in(d.object) || in(d.lights) || in(d.material) || in(d.point_lights) || in(d.spot_lights) ||
                in(d.shadow_data)) return true;
        }
        // the view constants of a multiview scope (read when it executes): [view_base, the highest view's matrix]
        if (pass.scope.view_mask && pass.scope.view_base < hi && lo < pass.scope.view_base + (size_t)(31 - __builtin_clz(pass.scope.view_mask)) * pass.scope.view_stride + 64) return true;
        // a transfer's buffers, read or written: a host write into either waits for it
        if (pass.xfer.kind && ((pass.xfer.span[0] && pass.xfer.span[0] < hi && lo < pass.xfer.span[1]) || (pass.xfer.span[2] && pass.xfer.span[2] < hi && lo < pass.xfer.span[3]))) return true;
    }
    return false;
}
static mirhi_result settle_readers(mirhi_device* dev, const uint8_t* lo, const uint8_t* hi) {
    std::vector<mirhi_cmd*> readers;
    {
        std::lock_guard<std::mutex> lk(dev->mu);
        for (mirhi_cmd* c : dev->cmds)
            // (`planned` is the recording the pending submissions were planned from and does not change while one is pending; `passes` may be
            // under re-recording by another host thread at this very moment)
            if ((c->pending || c->queued.load(std::memory_order_acquire) > 0) && recording_reads(c->planned, lo, hi)) readers.push_back(c);
    }
    for (mirhi_cmd* c : readers) { const mirhi_result r = settle_pending(c, false); if (r != MIRHI_OK) return r; }
    return MIRHI_OK;
}

#ifdef MIRHI_HOST_PROF
#include <x86intrin.h>
static unsigned long long g_hp[8]; static unsigned long long g_hp_n;
#define HP(k) do { const unsigned long long t_ = __rdtsc(); g_hp[k] += t_ - hp_t; hp_t = t_; } while (0)
#define HP_BEGIN unsigned long long hp_t = __rdtsc(); g_hp_n++
extern "C" void mirhi_debug_host_prof(void) { for (int k = 0; k < 8; k++) fprintf(stderr, "host prof [%d] %.1f cycles per call (%llu calls)\n", k, g_hp_n ? (double)g_hp[k] / (double)g_hp_n : 0.0, g_hp_n); }
#else
#define HP(k) do {} while (0)
#define HP_BEGIN do {} while (0)
#endif
// the plan stands for this device and workspace: no feedback of an earlier submission asks for clears, a bigger pool or another plan, and the tile split is
// the one it was built for
static bool plan_stands(const mirhi_cmd* cmd) {
    const mirhi_device* dev = cmd->dev;
    return cmd->plan_valid && !cmd->ws.grow_pool && !cmd->ws.replan && !cmd->ws.scope_bins.dirty && cmd->plan_split_rank == dev->split_rank && cmd->plan_split_world == dev->split_world &&
           cmd->plan_split_layout == dev->split_layout;
}
// the recording is the planned one but for the addresses of its colour targets: the host copy and both parities of every scope in the parameter block get the new ones
static mirhi_result retarget_color(mirhi_cmd* cmd) {
    mirhi_device* dev = cmd->dev;
    HIP_TRY(hipSetDevice(dev->ordinal));
    hipStream_t stream = dev->lanes[cmd->lane < dev->lanes.size() ? cmd->lane : 0];
    for (size_t pi = 0; pi < cmd->passes.size(); pi++) {
        uint8_t* target = const_cast<uint8_t*>(cmd->passes[pi].scope.color.ptr);
        cmd->plan[pi].color = target;
        for (uint32_t parity = 0; parity < 2; parity++) reinterpret_cast<PassParams*>(cmd->ws.pimage.data() + BlockLayout::scope_params(pi, parity))->color = target;
    }
    const mirhi_result r = pblock_commit(cmd->ws, stream);
    if (r != MIRHI_OK) { cmd->plan_valid = false; return r; }
    if (!cmd->ws.pblock_direct) { cmd->last_stream = stream; cmd->last_native = nullptr; cmd->pending = true; }     // (the copy is in the lane's stream)
    { std::lock_guard<std::mutex> lk(dev->mu); cmd->planned = cmd->passes; }
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_cmd_end(mirhi_cmd* cmd) {
    HP_BEGIN;
    REQUIRE_RECORDING(cmd);
    if (cmd->in_rendering) return fail(MIRHI_ERR_DEVICE, "Vulkan error: end() inside an active rendering scope");
    // The frame recorded last time, recorded again: plan, workspace and parameter block are what they have to be.  No HIP call, no synchronisation,
    // nothing uploaded.  Or the same frame into another swapchain image: the plan stands too, PassParams::color of every scope is rewritten.
    const bool unchanged = plan_stands(cmd) && same_recording(cmd->passes, cmd->planned);
    if (unchanged) HP(0);
    if (unchanged || (plan_stands(cmd) && cmd->plan.size() == cmd->passes.size() && cmd->ws.pimage.size() >= cmd->passes.size() * 2 * sizeof(PassParams) &&
                      same_recording(cmd->passes, cmd->planned, true))) {
        // only the status words of the previous submission are handed over and re-armed (a submission that is still pending reads the workspace and the
        // parameter block: wait for it -- a fenced loop has)
        mirhi_result r = settle_pending(cmd);
        if (r != MIRHI_OK) return r;
        HP(1);
        bool stands = true;
        if (cmd->ws.status_host && cmd->ws.any_status()) { HP(2); hand_over_status(cmd); HP(3); cmd->ws.clear_status(); HP(4); stands = plan_stands(cmd); }
        if (stands) {      // (else the status just handed over asked for clears or another plan: rebuild)
            if (!unchanged && (r = retarget_color(cmd)) != MIRHI_OK) return r;
            cmd->state = CMD_EXECUTABLE;
            return MIRHI_OK;
        }
    }
    mirhi_result r = build_plan(cmd);
    if (r != MIRHI_OK) { cmd->plan_valid = false; return r; }
    cmd->state = CMD_EXECUTABLE;
    return MIRHI_OK;
}

// Host-written parameter block (Workspace::pblock).  Fine-grained device memory is mapped into the host's address space; if the
// platform refuses either the allocation or the mapping, MIRHI_PARAM_UPLOAD=copy (or a failed allocation) selects plain device
// memory filled by stream-ordered copies from a pinned staging buffer.
static mirhi_result pblock_reserve(Workspace& w, size_t bytes) {
    if (w.pblock && w.pblock_bytes >= bytes) return MIRHI_OK;
    const size_t want = (bytes + 4095) & ~(size_t)4095;
    if (w.pblock) { (void)hipFree(w.pblock); w.pblock = nullptr; w.pblock_bytes = 0; }
    if (w.pstage) { (void)hipHostFree(w.pstage); w.pstage = nullptr; w.pstage_bytes = 0; }
    w.pshadow.clear();
    void* p = nullptr;
    const bool want_copy = getenv("MIRHI_PARAM_UPLOAD") && strcmp(getenv("MIRHI_PARAM_UPLOAD"), "copy") == 0;
    hipError_t e = want_copy ? hipErrorNotSupported : hipExtMallocWithFlags(&p, want, hipDeviceMallocFinegrained);
    w.pblock_direct = e == hipSuccess;
    if (e != hipSuccess) {
        (void)hipGetLastError();
        e = hipMalloc(&p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipMalloc(%zu) for the parameter block: %s", want, hipGetErrorString(e)); }
        void* h = nullptr;
        e = hipHostMalloc(&h, want, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: hipHostMalloc(%zu) for parameter staging: %s", want, hipGetErrorString(e)); }
        w.pstage = (uint8_t*)h; w.pstage_bytes = want;
    }
    w.pblock = (uint8_t*)p; w.pblock_bytes = want;
    return MIRHI_OK;
}
// Brings the block to `pimage`: nothing if it holds those bytes already.
static mirhi_result pblock_commit(Workspace& w, hipStream_t stream) {
    const size_t n = w.pimage.size();
    if (w.pshadow.size() == n && (n == 0 || memcmp(w.pshadow.data(), w.pimage.data(), n) == 0)) return MIRHI_OK;
    if (n) {
        if (w.pblock_direct) {
            // write-combined stores over the BAR, only the 64-byte pieces that differ from what the block holds (a frame loop changes a target address or a count) ...
            if (w.pshadow.size() == n) {
                for (size_t o = 0; o < n; o += 64) {
                    const size_t len = n - o < 64 ? n - o : 64;
                    if (memcmp(w.pshadow.data() + o, w.pimage.data() + o, len) != 0) memcpy(w.pblock + o, w.pimage.data() + o, len);
                }
            } else memcpy(w.pblock, w.pimage.data(), n);
            __builtin_ia32_sfence();                         // ... out of the write-combining buffers before any launch rings a doorbell
        } else {
            memcpy(w.pstage, w.pimage.data(), n);
            HIP_TRY(hipMemcpyAsync(w.pblock, w.pstage, n, hipMemcpyHostToDevice, stream));
            w.foreign = true;
        }
    }
    w.pshadow = w.pimage;
    return MIRHI_OK;
}

// ---- build_plan, step by step ----------------------------------------------------------------------
// 1. what a scope is and how it is rastered and binned (mirhi_scope.h), on its share of the tile rows
struct ScopePlan {
    uint32_t tiles_x, tiles_y, r0, r1, rstep;      // r0 / r1 / rstep: PassParams::tile_row_begin / _end / _step
    RenderArea area;                               // the scope's render area and the tiles it launches (mirhi_scope.h); a transfer has none
    size_t tris;                                   // the segment's own triangles
    ScopeClass cls; RasterMode mode; BinGeometry bins;
    size_t tiles() const { return (size_t)tiles_x * (r1 - r0); }      // the tiles bins, counters and page table are indexed by
    // ... and the tiles the scope launches, which the mode and the bins' densities are judged by: fewer under a partial render area
    size_t launched() const { return area.partial ? (size_t)area.tiles : tiles(); }
    // ... and the tiles raster_mode judges the density by: the ATTACHMENT's when the area is partial, as for the full-extent scope with a scissor that
    // such a scope replaces.  A scope's triangle count says nothing about how many of its triangles survive the cut to the area (C2's 10k triangles at
    // 4K against a 512 x 512 area: 2 %), and every triangle that crosses the area's edge is cut by the scissor and sits in the big list, which the
    // triangle-parallel variants stage slowly: judged by the launched tiles such a scope took 525-580 us where the sparse variant takes 58
    // (DESIGN_NOTES.md "Render areas").  The bins' fixed pages are still sized by the launched tiles.
    size_t density_tiles() const { return area.partial ? (size_t)tiles_x * tiles_y : tiles(); }
};
static ScopePlan plan_scope(const mirhi_device* dev, const RecordedPass& pass, const Workspace& w, const PlanKnobs& knobs) {
    ScopePlan s;
    s.tiles_x = (pass.scope.color.width + TILE - 1) / TILE; s.tiles_y = (pass.scope.color.height + TILE - 1) / TILE;
    { uint32_t count; split_rows(dev->split_layout, dev->split_rank, dev->split_world, s.tiles_y, &s.r0, &s.rstep, &count); s.r1 = s.r0 + count; }
    if (pass.scope.depth_only) { s.r0 = 0; s.r1 = s.tiles_y; s.rstep = 1; }      // every rank renders the whole depth image (include/mirhi.h, tile split)
    // (a transfer is not split: every rank moves what its own memory holds; one "tile" for the workspace's sizes, the launch's workgroups are fill_params')
    if (pass.xfer.kind) { s.tiles_x = 1u; s.tiles_y = 1u; s.r0 = 0u; s.r1 = 1u; s.rstep = 1u; }
    // The render area (validated by begin_rendering; never partial on a split device): its tile rows take the place of the band's -- bins, counters and
    // the raster grid are indexed by the owned row already --, its tile columns are a sub-range of the launch alone.  One evaluation per scope.
    s.area = RenderArea{};
    if (!pass.xfer.kind) {
        s.area = render_area(pass.scope.color.width, pass.scope.color.height, pass.scope.area);
        if (s.area.partial) { s.r0 = s.area.row_begin; s.r1 = s.area.row_end; s.rstep = 1; }
    }
    s.tris = pass.total_tris - pass.first_tri;
    s.cls = classify_scope(pass.state, pass.scope.clear_depth, pass.draws.data(), pass.draws.size(), pass.scope.depth_only, knobs, pass.sky.on != 0u, pass.xfer.kind != 0u, pass.scope.samples);
    s.mode = raster_mode(s.cls, s.density_tiles(), s.tris, w.spread, w.wide, knobs, s.area.partial);
    s.bins = bin_geometry(s.launched(), s.tris, pass.total_tris, s.mode.xcd_bins, w.pool_scale, knobs, s.tiles());
    return s;
}

// 2. the bin sets: growth, idle check and clears, once for both (rearm_workspace: the scopes' set; grow_multiview: the view slots').
// Buffers only ever grow, and a frame loop's do not: the steady state allocates nothing.  Counters and page table are cleared
// when they are new (or after a frame that went wrong on the device: BinSet::dirty) -- never otherwise: every kernel leaves
// them re-armed (raster_body: bin counters, table rows, pool counters, the other parity's big-list counter), and the fixed
// words of the counter block do not move when the tile count changes (CTR_*).
//
// Growth to `slots` slices of at least the strides `want`.  What growth costs is where the two sets differ, and that is `together`:
//   false (the scopes' set, one slot): each buffer grows on its own, and the set is dirty only when the table or the counters are new memory -- a
//         bigger pool or big list moves nothing that the kernels left armed;
//   true  (the view slots): a stride or the slot count that grew moves the slices, so all five buffers are sized anew and the set is dirty.
// A buffer whose stride is 0 is not allocated (the scopes' vertex output is sized with the other buffers that the scopes' contents decide: grow_scope_buffers).
static mirhi_result grow_bins(BinSet& b, size_t slots, const BinSet::Strides& want, bool together) {
    BinSet::Strides& s = b.stride;
    const bool grew = slots > b.slots || want.pages > s.pages || want.tiles > s.tiles || want.counter_words > s.counter_words || want.big_cap > s.big_cap || want.vs_bytes > s.vs_bytes;
    b.slots = (uint32_t)std::max<size_t>(slots, b.slots);
    s.pages = std::max(want.pages, s.pages); s.tiles = std::max(want.tiles, s.tiles); s.counter_words = std::max(want.counter_words, s.counter_words);
    s.big_cap = std::max(want.big_cap, s.big_cap); s.vs_bytes = std::max(want.vs_bytes, s.vs_bytes);
    const size_t n = b.slots, table_bytes = n * s.tiles * BIN_TABLE_ROW * sizeof(uint32_t), counters_bytes = n * s.counter_words * sizeof(uint32_t);
    const bool had = b.table && b.table_bytes >= table_bytes && b.counters && b.counters_bytes >= counters_bytes;
    if (together ? grew : !had) b.dirty = true;
    mirhi_result r;
    if ((r = grow(&b.pool, &b.pool_bytes, n * s.pages * BIN_PAGE_RECS * sizeof(BinRec))) != MIRHI_OK) return r;
    if ((r = grow(&b.table, &b.table_bytes, table_bytes)) != MIRHI_OK) return r;
    if ((r = grow(&b.counters, &b.counters_bytes, counters_bytes)) != MIRHI_OK) return r;
    if ((r = grow(&b.big, &b.big_bytes, n * s.big_cap * sizeof(BigRec))) != MIRHI_OK) return r;
    if (s.vs_bytes && (r = grow(&b.vs, &b.vs_bytes, n * s.vs_bytes)) != MIRHI_OK) return r;
    return MIRHI_OK;
}
// ... and the set's idle state: checked on request where the plan relies on it, restored by two clears where it is not known.  `which`: "" / "multiview ".
static mirhi_result rearm_bins(mirhi_cmd* cmd, BinSet& b, const char* which, hipStream_t stream, const PlanKnobs& knobs) {
    if (!b.dirty && knobs.verify_idle.set) {
        // Test hook: what the plan relies on instead of clearing -- every kernel leaves the workspace re-armed -- is checked here, on the
        // host: all bin and pool counters zero, the big-list counter of every slot's next parity zero, every page-table entry PAGE_EMPTY.
        HIP_TRY(hipStreamSynchronize(stream));
        const size_t words = b.stride.counter_words;
        std::vector<uint32_t> c(b.slots * words), t((size_t)b.slots * b.stride.tiles * BIN_TABLE_ROW);
        HIP_TRY(hipMemcpy(c.data(), b.counters, c.size() * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(t.data(), b.table, t.size() * 4, hipMemcpyDeviceToHost));
        size_t bad_c = 0, bad_t = 0;
        for (uint32_t j = 0; j < b.slots; j++)
            for (size_t i = 0; i < words; i++)       // (the last length of the slot's big list; the busy-tile counters of its last scope, read and re-armed by the next one)
                bad_c += (c[j * words + i] != 0u && i != (size_t)(CTR_BIG + (b.parity_of(j) ^ 1u)) && !(i >= CTR_ACTIVE && i < CTR_ACTIVE + 2u * 8u * 32u)) ? 1 : 0;
        for (uint32_t v : t) bad_t += v != PAGE_EMPTY ? 1 : 0;
        if (bad_c || bad_t) return fail(MIRHI_ERR_DEVICE, "Vulkan error: %sworkspace not idle between frames: %zu counter words, %zu page-table entries left set", which, bad_c, bad_t);
    }
    if (b.dirty) {
        HIP_TRY(hipMemsetAsync(b.table, 0xFF, b.table_bytes, stream));          // PAGE_EMPTY
        HIP_TRY(hipMemsetAsync(b.counters, 0, b.counters_bytes, stream));
        cmd->dev->foreign_writes++;
        b.parity = 0;
        b.dirty = false;
        cmd->last_stream = stream; cmd->last_native = nullptr; cmd->pending = true;      // (a submit on another stream or queue waits for the clears)
    }
    return MIRHI_OK;
}

// The scopes' set for the largest scope; the previous submission's status handed over; everything re-armed.
static mirhi_result rearm_workspace(mirhi_cmd* cmd, const std::vector<ScopePlan>& scopes, size_t max_tiles, hipStream_t stream, const PlanKnobs& knobs) {
    Workspace& w = cmd->ws;
    mirhi_result r;
    size_t max_pages = 0, max_big = 0;
    bool any_xcd_bins = false;
    for (const ScopePlan& s : scopes) { max_pages = std::max(max_pages, s.bins.pages); max_big = std::max<size_t>(max_big, s.bins.big_cap); any_xcd_bins |= s.mode.xcd_bins; }
    BinSet::Strides want;
    want.pages = max_pages ? max_pages : 1; want.tiles = max_tiles ? max_tiles : 1; want.big_cap = max_big ? max_big : 1;
    // fixed words (big-list and pool counters), then the bin counters: one per tile -- per tile and XCD in scopes with per-XCD bins -- 64 bytes apart
    want.counter_words = CTR_BINS + (any_xcd_bins ? 8 : 1) * max_tiles * (size_t)BIN_COUNT_STRIDE;
    if ((r = grow_bins(w.scope_bins, 1, want, false)) != MIRHI_OK) return r;
    w.xcd_tiles_last = (!scopes.empty() && scopes.back().mode.xcd_bins) ? (uint32_t)scopes.back().tiles() : 0u;
    if (knobs.always_clear.set) w.scope_bins.dirty = true;             // (A/B runs: the round-2 behaviour, two memsets per recording)
    if (!w.status_host) {
        HIP_TRY(hipHostMalloc((void**)&w.status_host, Workspace::STATUS_WORDS * 4u, hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void**)&w.status_dev, w.status_host, 0));
    }
    w.stats_params_valid = false;
    hand_over_status(cmd);          // an earlier submission's status is not lost to the re-arm below (and may ask for a bigger pool: before the flags are cleared)
    w.grow_pool = false; w.replan = false;
    w.clear_status();
    const bool clears = w.scope_bins.dirty;
    if ((r = rearm_bins(cmd, w.scope_bins, "", stream, knobs)) != MIRHI_OK) return r;
    if (clears) w.view_bins.dirty = true;      // (whatever asked for the clears asked for those of the view slots too: grow_multiview)
    return MIRHI_OK;
}

// 3. vertex pre-pass jobs of one scope: one per distinct (vertex range, camera, object, program class).  The recorded descriptors stay as recorded
// (plan cache); `draws` are copies with the plan's fields, vs_out / vs_attr as offset + 1 into the scope's output (patched to pointers in step 4)
struct VertexPlan { std::vector<VsJob> jobs; std::vector<size_t> out_off; std::vector<DrawDesc> draws; size_t out_bytes = 0; };
static VertexPlan vertex_jobs(const RecordedPass& pass) {
    VertexPlan v;
    v.draws = pass.draws;
    uint32_t slots = 0;
    for (size_t di = 0; di < pass.draws.size(); di++) {
        DrawDesc& dd = v.draws[di];
        dd.vs_words = 0; dd.vs_out = nullptr; dd.vs_attr = nullptr;
        if (dd.program == MIRHI_PROGRAM_TRIANGLE) continue;
        const uint32_t words = dd.program == MIRHI_PROGRAM_SHADOW ? 1u : (dd.program == MIRHI_PROGRAM_MODEL ? 3u : 5u);   // (SHADOW: the clip stream only)
        const uint64_t vbb = pass.draw_vb_bytes[di];
        const uint64_t vsz = dd.program == MIRHI_PROGRAM_SHADOW ? 12u : 48u;
        const uint32_t count = vbb >= vsz ? (uint32_t)((vbb - vsz) / dd.stride + 1) : 0u;
        size_t found = SIZE_MAX;
        for (size_t j = 0; j < v.jobs.size(); j++) {
            const VsJob& J = v.jobs[j];
            if (J.vb == dd.vb && J.camera == dd.camera && J.object == dd.object && J.stride == dd.stride && J.words >= words && (J.words == 1u) == (words == 1u) && J.count >= count) { found = j; break; }
        }
        if (found == SIZE_MAX) {
            VsJob j{};
            j.vb = dd.vb; j.camera = dd.camera; j.object = dd.object; j.stride = dd.stride; j.count = count;
            j.words = words; j.slot_base = slots;
            slots += (count + GEOM_THREADS - 1) / GEOM_THREADS * GEOM_THREADS;
            v.jobs.push_back(j); v.out_off.push_back(v.out_bytes);
            v.out_bytes += vs_attr_offset(count) + (((size_t)count * (words - 1u) * 16 + 255) & ~(size_t)255);      // clip stream, then the attribute stream
            found = v.jobs.size() - 1;
        }
        dd.vs_words = v.jobs[found].words;
        dd.vs_out = (const void*)(uintptr_t)(v.out_off[found] + 1);
        dd.vs_attr = (const void*)(uintptr_t)(v.out_off[found] + vs_attr_offset(v.jobs[found].count) + 1);
    }
    return v;
}

// ... and the buffers whose size the scopes' contents decide: vertex output, depth hand-over, ordered records, flat colours, primitive -> draw
static mirhi_result grow_scope_buffers(Workspace& w, const std::vector<RecordedPass>& passes, const std::vector<ScopePlan>& scopes, const std::vector<VertexPlan>& vertex) {
    mirhi_result r;
    size_t vs_bytes = 0, carry = 0, ord = 0, flat_tris = 0, pd = 0;
    for (size_t pi = 0; pi < passes.size(); pi++) {
        const RecordedPass& pass = passes[pi];
        vs_bytes = std::max(vs_bytes, vertex[pi].out_bytes);
        if ((pass.carry_in || pass.carry_out) && !pass.scope.depth.ptr) carry = std::max(carry, (size_t)pass.scope.color.width * pass.scope.color.height * 4);
        if (scopes[pi].cls.ordered) ord = std::max(ord, scopes[pi].tris * sizeof(TriRec));
        if (scopes[pi].cls.tri_prog && pass.scope.color.format == MIRHI_FORMAT_B8G8R8A8_SRGB) flat_tris = std::max<size_t>(flat_tris, pass.total_tris);
        if (pass.draws.size() > 1) pd = std::max(pd, scopes[pi].tris);
    }
    if ((r = grow(&w.scope_bins.vs, &w.scope_bins.vs_bytes, vs_bytes ? vs_bytes : 256)) != MIRHI_OK) return r;
    w.scope_bins.stride.vs_bytes = w.scope_bins.vs_bytes;      // (the one slot's)
    if (carry && (r = grow(&w.carry_depth, &w.carry_depth_bytes, carry)) != MIRHI_OK) return r;
    if (ord && (r = grow(&w.ordered, &w.ordered_bytes, ord)) != MIRHI_OK) return r;
    if (flat_tris && (r = grow(&w.flat_color, &w.flat_color_bytes, flat_tris * 4)) != MIRHI_OK) return r;
    if (pd && (r = grow(&w.prim_draw, &w.prim_draw_bytes, pd * 4)) != MIRHI_OK) return r;
    return MIRHI_OK;
}

// ... and the view slots of the command buffer's multiview scopes (Workspace::view_bins): slices for the most views, each sized for the largest such scope.  A
// slice that moves (any of the strides grew) or was never used is cleared; otherwise the kernels left it re-armed, which MIRHI_VERIFY_IDLE checks as it does
// for the scopes' set.  A command buffer without a multiview scope leaves the set as it is.
static mirhi_result grow_multiview(mirhi_cmd* cmd, const std::vector<ScopePlan>& scopes, const std::vector<VertexPlan>& vertex, hipStream_t stream, const PlanKnobs& knobs) {
    Workspace& w = cmd->ws;
    size_t slots = 0, pages = 0, tiles = 0, big = 0, vs = 0;
    for (size_t pi = 0; pi < cmd->passes.size(); pi++) {
        if (!cmd->passes[pi].scope.view_mask) continue;
        slots = std::max<size_t>(slots, multiview_count(cmd->passes[pi].scope.view_mask));
        pages = std::max(pages, scopes[pi].bins.pages); tiles = std::max(tiles, scopes[pi].tiles());
        big = std::max<size_t>(big, scopes[pi].bins.big_cap); vs = std::max(vs, vertex[pi].out_bytes);
    }
    if (!slots) return MIRHI_OK;
    // One bin counter per tile, without the scopes' set's factor of 8 for per-XCD bins: a multiview scope never has them.  It is depth-only (open_scope: no
    // colour target), so classify_scope sets own_family (mirhi_scope.h:284, "c.own_family = depth_only || ..."), which makes raster_mode's mesh_only false
    // (:316), which leaves teams at 1 whatever MIRHI_RASTER_TEAMS says (:318), and ":321  m.xcd_bins = m.teams == 2u && ..." is false.
    BinSet::Strides want;
    want.pages = pages; want.tiles = tiles; want.counter_words = CTR_BINS + tiles * (size_t)BIN_COUNT_STRIDE; want.big_cap = big;
    want.vs_bytes = std::max<size_t>(256, (vs + 255) & ~(size_t)255);
    mirhi_result r;
    if ((r = grow_bins(w.view_bins, slots, want, true)) != MIRHI_OK) return r;
    return rearm_bins(cmd, w.view_bins, "multiview ", stream, knobs);
}

// 4. one scope's parameters from its class, mode, bins and the workspace (the bin set's slot, the draws and the vertex jobs are placed by place_scope)
static PassParams fill_params(const RecordedPass& pass, const ScopePlan& s, const RasterMode& mode, const Workspace& w, size_t max_tiles, unsigned long long* frag_stats) {
    const ScopeHeader::Target& ci = pass.scope.color;
    PassParams P;
    memset(&P, 0, sizeof P);
    P.width = ci.width; P.height = ci.height;
    P.tiles_x = s.tiles_x; P.tiles_y = s.tiles_y; P.tile_row_begin = s.r0; P.tile_row_end = s.r1; P.tile_row_step = s.rstep;
    // (a transfer has no area: its kernels read none of these words)
    P.area_x0 = s.area.x; P.area_y0 = s.area.y; P.area_w = s.area.valid ? s.area.w : ci.width; P.area_h = s.area.valid ? s.area.h : ci.height;
    P.area_partial = s.area.partial ? 1u : 0u;
    P.tile_col_begin = s.area.partial ? s.area.col_begin : 0u; P.tile_cols = s.area.partial ? s.area.col_end - s.area.col_begin : s.tiles_x;
    P.num_draws = (uint32_t)pass.draws.size(); P.total_tris = pass.total_tris;
    set_raster_choice(P, s.cls, mode, pass.state, w.ordered, pass.first_tri, pass.total_tris);
    memcpy(P.clear_color, pass.scope.clear_color, sizeof P.clear_color);
    {   // sRGB OETF + UNORM8 of the clear colour, BGRA byte order (swapchain.rs:561-570)
        auto sat = [](float c) { return c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f; };
        auto enc = [&](float c) { c = sat(c); float e = c <= 0.0031308f ? 12.92f * c : 1.055f * std::pow(c, 1.0f / 2.4f) - 0.055f; return (uint32_t)std::nearbyint(sat(e) * 255.0f); };
        P.clear_packed = enc(P.clear_color[2]) | (enc(P.clear_color[1]) << 8) | (enc(P.clear_color[0]) << 16) |
                         ((uint32_t)std::nearbyint(sat(P.clear_color[3]) * 255.0f) << 24);
    }
    P.color_load = pass.scope.color_load_op == MIRHI_LOAD_OP_LOAD ? 1u : 0u;
    P.color_format = ci.format;
    P.color = const_cast<uint8_t*>(ci.ptr);
    if (pass.scope.depth.ptr) {
        P.depth = (float*)const_cast<uint8_t*>(pass.scope.depth.ptr);
        P.depth_load = pass.scope.depth_load_op == MIRHI_LOAD_OP_LOAD ? 1u : 0u;
        P.depth_store = pass.scope.depth_store_op == MIRHI_STORE_OP_STORE ? 1u : 0u;
    } else if (pass.carry_in || pass.carry_out) {
        P.depth = w.carry_depth;               // no depth attachment: the segments of the scope hand depth over here
    }
    if (pass.carry_in) P.depth_load = 1u;
    if (pass.carry_out) P.depth_store = 1u;
    P.prim_out = (uint32_t*)const_cast<uint8_t*>(pass.scope.prim.ptr);
    P.bin_cap = s.bins.bin_cap;
    P.pool_dyn_base = s.bins.fixed_pages;
    P.fixed_recs = s.bins.fixed_per_tile * BIN_PAGE_RECS;
    P.big_cap = s.bins.big_cap;
    P.status = w.status_dev;
    P.frag_stats = frag_stats;
    P.first_prim = pass.first_tri;
    P.prim_draw = pass.draws.size() > 1 ? w.prim_draw : nullptr;
    // (a multisampled scope averages linear colours: no packed flat colours)
    P.flat_color = (s.cls.tri_prog && ci.format == MIRHI_FORMAT_B8G8R8A8_SRGB && pass.scope.samples == 1u) ? w.flat_color : nullptr;
    P.resolve_flat_only = (P.flat_color && !P.depth_load && P.color_format != 2u && !P.prim_out && !(P.depth && P.depth_store)) ? 1u : 0u;
    P.sub_cap = s.bins.sub_cap;                                       // (the bins are those the workspace was sized for: s.mode, not `mode`)
    P.count_stride = s.mode.xcd_bins ? (uint32_t)max_tiles : 0u;
    P.depth_only = pass.scope.depth_only ? 1u : 0u;
    if (P.ibl) {
        P.ibl_irradiance = (const float*)pass.scope.ibl.irradiance; P.ibl_prefiltered = (const float*)pass.scope.ibl.prefiltered; P.ibl_lut = (const float*)pass.scope.ibl.lut;
        P.ibl_irr_size = pass.scope.ibl.irr_size; P.ibl_pre_size = pass.scope.ibl.pre_size; P.ibl_pre_levels = pass.scope.ibl.pre_levels; P.ibl_lut_size = pass.scope.ibl.lut_size;
        P.ibl_seamless = pass.scope.ibl.seamless;
    }
    if (P.sky) {
        const RecordedPass::SkyDraw& k = pass.sky;
        P.sky_visible = k.visible; P.sky_size = k.size; P.sky_levels = k.levels; P.sky_env = (const float*)k.env; P.sky_seamless = k.seamless;
        memcpy(P.sky_a, k.a, sizeof P.sky_a); memcpy(P.sky_b, k.b, sizeof P.sky_b); memcpy(P.sky_scissor, k.scissor, sizeof P.sky_scissor);
        for (int i = 0; i < 3; i++) P.sky_e0[i] = k.e0[i];
        memcpy(P.sky_pos0, k.pos0, sizeof P.sky_pos0); memcpy(P.sky_posx, k.posx, sizeof P.sky_posx); memcpy(P.sky_posy, k.posy, sizeof P.sky_posy);
        P.sky_depth_bits = k.depth_bits; P.sky_compare = k.compare; P.sky_write = k.write; P.sky_prim = k.prim;
    }
    if (pass.xfer.kind) {      // (xfer_regions: build_plan places them in the parameter block)
        const RecordedPass::Transfer& t = pass.xfer;
        P.xfer = t.kind; P.xfer_count = t.count; P.xfer_src_format = t.src_format; P.xfer_dst_format = t.dst_format; P.xfer_groups = t.groups;
        memcpy(P.xfer_color, t.color, sizeof P.xfer_color);
        P.tiles_x = t.grid;      // the launch's workgroups (raster_variant: a 1-D grid)
    }
    return P;
}

// `P` for big-list parity `parity` of a slot's counter block (BinSet::Slot::counters): the scope appends large triangles to counter `parity` and counts its busy
// tiles in that half, and re-arms the other ones for the scope that follows on the slot
static PassParams with_parity(PassParams P, uint32_t* counters, uint32_t parity) {
    P.big_count = counters + CTR_BIG + parity;
    P.big_count_next = counters + CTR_BIG + (parity ^ 1u);
    P.active = counters + CTR_ACTIVE + parity * 8u * 32u;
    P.active_prev = counters + CTR_ACTIVE + (parity ^ 1u) * 8u * 32u;
    return P;
}

// Places a scope -- or, with `camera`, one view of a multiview scope, which differs in the light matrix's address and the slot alone -- into the parameter
// image: P bound to slot `b` of a bin set; the plan's draws with vs_out / vs_attr as pointers into the slot's vertex output and their slot_base; the vertex
// jobs; and the two parity copies of P at `params_at` (the kernels read their parameters from the block).  `at`: where the draws and the jobs go (bytes
// into the block), moved on behind them.  Returns P as the host keeps it.
struct BlockCursor { size_t draws, jobs; };
static PassParams place_scope(Workspace& w, PassParams P, const BinSet::Slot& b, const VertexPlan& v, const float* camera, size_t params_at, BlockCursor& at) {
    P.bin_pool = b.pool; P.bin_table = b.table; P.bin_count = b.counters + CTR_BINS; P.pool_next = b.counters + CTR_POOL;
    P.pool_dyn_pages = (uint32_t)((b.pages - P.pool_dyn_base) / 8);      // per XCD
    P.big_recs = b.big; P.big_count = b.counters + CTR_BIG; P.big_count_next = b.counters + CTR_BIG + 1;
    P.draws = reinterpret_cast<DrawDesc*>(w.pblock + at.draws);
    DrawDesc* const img_draws = reinterpret_cast<DrawDesc*>(w.pimage.data() + at.draws);
    uint32_t slots = 0;
    for (size_t di = 0; di < v.draws.size(); di++) {
        DrawDesc dd = v.draws[di];
        if (camera) dd.camera = camera;
        if (dd.vs_words) { dd.vs_out = b.vs + ((size_t)(uintptr_t)dd.vs_out - 1); dd.vs_attr = b.vs + ((size_t)(uintptr_t)dd.vs_attr - 1); }      // (vertex_jobs: offset + 1)
        dd.slot_base = slots; slots += (dd.tri_count + GEOM_THREADS - 1) / GEOM_THREADS * GEOM_THREADS;
        img_draws[di] = dd;
    }
    P.total_slots = slots;
    at.draws += v.draws.size() * sizeof(DrawDesc);
    P.vs_jobs = reinterpret_cast<VsJob*>(w.pblock + at.jobs);
    P.num_vs_jobs = (uint32_t)v.jobs.size();
    VsJob* const img_jobs = reinterpret_cast<VsJob*>(w.pimage.data() + at.jobs);
    for (size_t k = 0; k < v.jobs.size(); k++) {
        VsJob job = v.jobs[k];
        if (camera) job.camera = camera;
        job.out = b.vs + v.out_off[k];
        P.vs_total_slots = job.slot_base + (job.count + GEOM_THREADS - 1) / GEOM_THREADS * GEOM_THREADS;
        img_jobs[k] = job;
    }
    at.jobs += v.jobs.size() * sizeof(VsJob);
    for (uint32_t parity = 0; parity < 2; parity++) {
        const PassParams Q = with_parity(P, b.counters, parity);
        memcpy(w.pimage.data() + params_at + parity * sizeof(PassParams), &Q, sizeof Q);
    }
    return P;
}

// Outside the C ABI (not in include/mirhi.h): how often this process has built a launch plan -- what end() of an unchanged recording does not do.
static std::atomic<uint64_t> g_plan_builds{0};
extern "C" uint64_t mirhi_debug_plan_builds(void) { return g_plan_builds.load(std::memory_order_relaxed); }

static mirhi_result build_plan(mirhi_cmd* cmd, bool in_submit) {
    g_plan_builds.fetch_add(1, std::memory_order_relaxed);
    const PlanKnobs knobs = PlanKnobs::read();
    mirhi_device* dev = cmd->dev;
    HIP_TRY(hipSetDevice(dev->ordinal));
    if (cmd->lane >= dev->lanes.size()) cmd->lane = 0;
    hipStream_t stream = dev->lanes[cmd->lane];
    cmd->plan_valid = false;
    { mirhi_result rs = settle_pending(cmd, in_submit); if (rs != MIRHI_OK) return rs; }
    Workspace& w = cmd->ws;
    const size_t n = cmd->passes.size();
    {
        uint64_t tris_now = 0;
        for (auto& pass : cmd->passes) tris_now += pass.total_tris - pass.first_tri;
        if (w.spread && (tris_now > 2 * w.spread_tris || 2 * tris_now < w.spread_tris)) w.spread = false;
    }
    mirhi_result r;
    std::vector<ScopePlan> scopes;
    size_t total_draws = 0, max_tiles = 0, total_regions = 0;
    for (const RecordedPass& pass : cmd->passes) {
        scopes.push_back(plan_scope(dev, pass, w, knobs));
        // (begin_rendering refuses it; a device split after the recording is met here)
        if (scopes.back().area.partial && dev->split_world > 1) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a partial render area on a split device");
        if (pass.scope.samples != 1u && dev->split_world > 1) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a multisampled scope on a split device");
        if (pass.scope.samples != 1u && (dev->profiling & MIRHI_PROFILE_FRAGMENTS)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: fragment statistics of a multisampled scope");
        if (pass.scope.view_mask && dev->split_world > 1) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: a multiview scope on a split device");
        if (pass.scope.view_mask && (dev->profiling & MIRHI_PROFILE_FRAGMENTS)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unsupported: fragment statistics of a multiview scope");
        total_draws += pass.draws.size();
        total_regions += pass.xfer_regions.size();
        max_tiles = std::max(max_tiles, scopes.back().tiles());
    }
    if ((r = rearm_workspace(cmd, scopes, max_tiles, stream, knobs)) != MIRHI_OK) return r;
    std::vector<VertexPlan> vertex;
    size_t jobs_total = 0;
    for (const RecordedPass& pass : cmd->passes) { vertex.push_back(vertex_jobs(pass)); jobs_total += vertex.back().jobs.size(); }
    if ((r = grow_scope_buffers(w, cmd->passes, scopes, vertex)) != MIRHI_OK) return r;
    if ((r = grow_multiview(cmd, scopes, vertex, stream, knobs)) != MIRHI_OK) return r;
    // the parameter block (BlockLayout)
    size_t view_slots = 0, view_draws = 0, view_jobs = 0;
    for (size_t pi = 0; pi < n; pi++)
        if (const uint32_t views = multiview_count(cmd->passes[pi].scope.view_mask)) { view_slots += views; view_draws += views * cmd->passes[pi].draws.size(); view_jobs += views * vertex[pi].jobs.size(); }
    const BlockLayout L = w.layout = block_layout(n, total_draws, total_regions, jobs_total, view_slots, view_draws, view_jobs);
    if ((r = pblock_reserve(w, L.bytes ? L.bytes : 256)) != MIRHI_OK) return r;
    w.params = reinterpret_cast<PassParams*>(w.pblock);
    w.pimage.assign(L.bytes, 0);

    size_t regions_at = L.regions, views_done = 0;
    BlockCursor scope_at{L.draws, L.jobs}, view_at{L.view_draws, L.view_jobs};
    w.wide_eligible = false;
    cmd->plan.clear(); cmd->plan_programs.clear(); cmd->plan_tris = 0;
    cmd->plan_views.clear(); cmd->plan_view_params.clear();
    for (size_t pi = 0; pi < n; pi++) {
        const ScopePlan& s = scopes[pi];
        const VertexPlan& v = vertex[pi];
        const RecordedPass& pass = cmd->passes[pi];
        // (the mode is evaluated again, not kept from step 1: hand_over_status in between may have changed w.spread / w.wide)
        const RasterMode mode = raster_mode(s.cls, s.density_tiles(), s.tris, w.spread, w.wide, knobs, s.area.partial);
        w.wide_eligible |= mode.wide_eligible;
        PassParams P = fill_params(pass, s, mode, w, max_tiles, dev->frag_stats);
        if (P.xfer) {
            P.xfer_regions = reinterpret_cast<const XferRegion*>(w.pblock + regions_at);
            memcpy(w.pimage.data() + regions_at, pass.xfer_regions.data(), pass.xfer_regions.size() * sizeof(XferRegion));
            regions_at += pass.xfer_regions.size() * sizeof(XferRegion);
        }
        // copy `parity` of scope pi appends large triangles to counter `parity` and re-arms the other one for the scope that follows on the scopes' bins
        cmd->plan.push_back(place_scope(w, P, w.scope_bins.slot(0), v, nullptr, L.scope_params(pi, 0), scope_at));
        cmd->plan_programs.push_back(s.cls.programs);
        cmd->plan_tris += s.tris;
        // A multiview scope: the same once per view slot -- depth base = the view's layer, status words and bins = the slot's (Workspace::view_bins), the light
        // matrix = the view's.  (plan[pi] itself stays: the host's idea of the scope's launch shape; its device copies are not launched.)
        mirhi_cmd::ViewSet vset;
        if (pass.scope.view_mask) {
            MultiviewSlot slot[MAX_BATCH];
            vset.count = multiview_slots(pass.scope.view_mask, pass.scope.color.width, pass.scope.color.height, 0u, pass.scope.view_stride, slot);
            vset.first = views_done;
            for (uint32_t j = 0; j < vset.count; j++) {
                const BinSet::Slot b = w.view_bins.slot(j);
                PassParams V = P;
                V.depth = reinterpret_cast<float*>(const_cast<uint8_t*>(pass.scope.depth.ptr) + slot[j].layer_offset);
                V.status = w.status_dev + Workspace::STATUS_VIEWS + 4u * j;
                V = place_scope(w, V, b, v, reinterpret_cast<const float*>(pass.scope.view_base + slot[j].matrix_offset), L.slot_params(views_done + j, 0), view_at);
                cmd->plan_view_params.push_back(with_parity(V, b.counters, 0u));      // (the host's copy is the parity-0 one)
            }
            views_done += vset.count;
        }
        cmd->plan_views.push_back(vset);
    }
    // 5. commit
    if ((r = pblock_commit(w, stream)) != MIRHI_OK) return r;
    if (!w.pblock_direct) { cmd->last_stream = stream; cmd->last_native = nullptr; cmd->pending = true; }     // (the copy is in the lane's stream)
    { std::lock_guard<std::mutex> lk(dev->mu); cmd->planned = cmd->passes; }      // (settle_readers scans `planned` of pending command buffers under this lock)
    cmd->plan_split_rank = dev->split_rank; cmd->plan_split_world = dev->split_world; cmd->plan_split_layout = dev->split_layout;
    cmd->plan_valid = true;
    dev->stats.workspace_bytes = w.bytes();
    return MIRHI_OK;
}

// Outside the C ABI (not in include/mirhi.h) and without a HIP call: what build_plan decides for one scope -- class, raster mode (one evaluation),
// bins -- and the kernel, grid and block that raster_variant then gives at 5 x 4 tiles.  The environment is read as build_plan reads it.
// in: DepthState key_set, test, compare, write, discard, blend enable; clear-depth float bits; depth_only; tiles; triangles; spread; wide; pool_scale;
// allow_wide; number of draws (at most 4); per draw: program, shadow kind 0 / 1 / 2 / 3 (3: blended cascades), bit 0 "has a mip chain or an sRGB texture" | bit 1 "texture 0 has sampler state" |
// bit 2 "texture 1 has sampler state".
// out: the key's eight words; ordered, masked_plain, tri_prog, shadowed, ibl, own_family, programs; tp_max_area, teams, wide_eligible, xcd_bins, wide,
// xcd_swizzle; bin_cap, sub_cap, fixed_per_tile, fixed_pages, pool pages (low, high word), big_cap; grid x, y, z, block.
extern "C" int mirhi_debug_raster_choice(const uint32_t in[12], char* name, uint32_t name_len, uint32_t grid_block[4]);
extern "C" int mirhi_debug_scope_plan(const uint32_t* in, uint32_t* out, char* name, uint32_t name_len) {
    static float some_map; static TriRec some_recs;
    const PlanKnobs knobs = PlanKnobs::read();
    DepthState s;
    s.key_set = in[0] != 0u; s.test = in[1]; s.compare = in[2]; s.write = in[3]; s.discard = in[4]; s.blend[0] = in[5];
    float clear_depth; memcpy(&clear_depth, &in[6], 4);
    const uint32_t n = in[14];
    if (n > 4u) return -1;
    DrawDesc draws[4];
    memset(draws, 0, sizeof draws);
    for (uint32_t i = 0; i < n; i++) {
        draws[i].program = in[15 + 3 * i];
        if (in[16 + 3 * i]) { draws[i].shadow_map = &some_map; draws[i].shadow_layers = in[16 + 3 * i] >= 2u ? 4u : 0u; draws[i].csm_blend = in[16 + 3 * i] == 3u ? 0.5f : 0.0f; }
        draws[i].tex_any_mips = in[17 + 3 * i] & 1u;
        draws[i].tex_sampler = ((in[17 + 3 * i] >> 1) & 1u) | (((in[17 + 3 * i] >> 2) & 1u) << 6);
    }
    const ScopeClass c = classify_scope(s, clear_depth, draws, n, in[7] != 0u, knobs, n == 1u && draws[0].program == (uint32_t)MIRHI_PROGRAM_SKYBOX);      // (a SKYBOX draw is a segment of its own)
    const RasterMode m = raster_mode(c, in[8], in[9], in[10] != 0u, in[11], knobs);
    const BinGeometry g = bin_geometry(in[8], in[9], in[9], m.xcd_bins, in[12], knobs);
    const uint32_t words[28] = {c.key.clear_depth_bits, c.key.pred, c.key.zflip, c.key.zmask, c.key.idflip, c.key.strict, c.key.init_zk, c.key.init_idk,
                                c.ordered, c.masked_plain, c.tri_prog, c.shadowed, c.ibl, c.own_family, c.programs,
                                m.tp_max_area, m.teams, m.wide_eligible, m.xcd_bins, m.wide, m.xcd_swizzle,
                                g.bin_cap, g.sub_cap, g.fixed_per_tile, g.fixed_pages, (uint32_t)g.pages, (uint32_t)((uint64_t)g.pages >> 32), g.big_cap};
    memcpy(out, words, sizeof words);
    PassParams P{};
    set_raster_choice(P, c, m, s, &some_recs, 0u, in[9]);
    const uint32_t choice[12] = {c.programs, in[13], P.pred, P.zflip, P.zmask, P.tp_max_area, P.raster_teams, P.raster_wide, P.alpha_scope, P.xcd_swizzle, P.ordered_recs ? 1u : 0u, 0u};
    return mirhi_debug_raster_choice(choice, name, name_len, out + 28);
}
// ... what render_area (mirhi_scope.h) decides for an attachment of in[0] x in[1] pixels and the area in[2 .. 5] (x, y, width, height as int32).  Returns 0 and
// out: x, y, w, h, partial, col_begin, col_end, row_begin, row_end, edge_partial, tiles, index_tiles -- or -1 for an invalid area, with the message
// begin_rendering refuses it with in `msg` (may be null).  No HIP call.
extern "C" int mirhi_debug_render_area(const int32_t in[6], uint32_t out[12], char* msg, uint32_t msg_len) {
    if (in[0] < 0 || in[1] < 0) return -2;
    const RenderArea a = render_area((uint32_t)in[0], (uint32_t)in[1], in + 2);
    if (!a.valid) {
        if (msg && msg_len) render_area_message(msg, msg_len, in + 2, (uint32_t)in[0], (uint32_t)in[1]);
        return -1;
    }
    const uint32_t words[12] = {a.x, a.y, a.w, a.h, a.partial, a.col_begin, a.col_end, a.row_begin, a.row_end, a.edge_partial, a.tiles, a.index_tiles};
    memcpy(out, words, sizeof words);
    if (msg && msg_len) msg[0] = 0;
    return 0;
}
// ... and what mirhi_submit.h decides about a submit, a scope of it and the wide feedback (the words: submit_words there)
extern "C" int mirhi_debug_submit_path(const uint32_t* in, uint32_t* out) { return submit_words(in, out); }

// ------------------------------------------------------------------------------------------------
// submit + fences
// ------------------------------------------------------------------------------------------------
// Statistics pass: device copies of the command buffer's scope parameters (both parities) whose primitive-id image is the
// workspace's own, built the first time a recorded command buffer is submitted with MIRHI_PROFILE_FRAGMENTS.
static mirhi_result stats_params_for(mirhi_cmd* c) {
    Workspace& w = c->ws;
    if (w.stats_params_valid) return MIRHI_OK;
    size_t pixels = 0;
    for (const PassParams& P : c->plan) pixels = std::max(pixels, (size_t)P.width * P.height);
    mirhi_result r;
    if ((r = grow(&w.stats_prim, &w.stats_prim_bytes, (pixels ? pixels : 1) * 4)) != MIRHI_OK) return r;
    if ((r = grow(&w.stats_params, &w.stats_params_bytes, (c->plan.size() ? c->plan.size() : 1) * 2 * sizeof(PassParams))) != MIRHI_OK) return r;
    std::vector<PassParams> copies;
    for (const PassParams& P0 : c->plan)
        for (uint32_t parity = 0; parity < 2; parity++) {
            PassParams P = with_parity(P0, w.scope_bins.slot(0).counters, parity);      // (in the order of the block's copies: BlockLayout::scope_params)
            P.prim_out = w.stats_prim;
            P.resolve_flat_only = 0u;
            copies.push_back(P);
        }
    if (!copies.empty()) {
        c->dev->foreign_writes++;
        HIP_TRY(hipMemcpyAsync(w.stats_params, copies.data(), copies.size() * sizeof(PassParams), hipMemcpyHostToDevice, c->dev->stream));
        HIP_TRY(hipStreamSynchronize(c->dev->stream));
    }
    w.stats_params_valid = true;
    return MIRHI_OK;
}

// Outside the C ABI (not in include/mirhi.h) and without a HIP call: what a 4x multisampled scope refuses (mirhi_scope.h), as words.  in[0] says what is asked:
// 0  a sample count: in[1].  1  a scope: the words of MsaaScopeFacts in their order, from in[1].  2  a draw: blend enable, discard, depth test, depth write,
// compare op, program, "samples a shadow map or cascades", "the segment holds draws of another depth state".  3  the variant of a 5 x 4 tile scope: programs,
// zflip, zmask, samples -> msg: the kernel's name, out of the launch table (mirhi_debug_raster_choice knows no sample count).
// Returns 0 (accepted; msg empty), 1 (refused; msg: the words behind "Invalid handle: "), -1 for words it cannot take.
extern "C" int mirhi_debug_msaa(const uint32_t* in, char* msg, uint32_t msg_len) {
    const char* why = nullptr;
    if (in[0] == 0u) why = msaa_sample_count_refusal(in[1]);
    else if (in[0] == 1u) {
        MsaaScopeFacts f;
        static_assert(sizeof(MsaaScopeFacts) % 4 == 0, "MsaaScopeFacts is made of 32-bit words");
        memcpy(&f, in + 1, sizeof f);
        why = msaa_scope_refusal(f);
    } else if (in[0] == 2u) {
        DepthState s;
        s.key_set = true; s.blend[0] = in[1]; s.discard = in[2]; s.test = in[3]; s.write = in[4]; s.compare = in[5];
        why = msaa_draw_refusal(s, (int32_t)in[6], in[7] != 0u, in[8] != 0u);
    } else if (in[0] == 3u) {
        PassParams P{};
        P.tiles_x = 5u; P.tile_row_end = 4u; P.tile_row_step = 1u; P.zflip = in[2]; P.zmask = in[3]; P.samples = in[4];
        const RasterVariant v = raster_variant(P, in[1], true);
        snprintf(msg, msg_len, "%s family %u progs %u keyed %u tp %u grid %u %u block %u batched %u", v.family == RASTER_MSAA ? "msaa" : "other", (uint32_t)v.family, v.progs, v.keyed,
                 v.tp, v.grid[0], v.grid[1], v.block, v.batched_form);
        return 0;
    } else return -1;
    snprintf(msg, msg_len, "%s", why ? why : "");
    return why ? 1 : 0;
}

// ... and what a multiview depth scope refuses and plans (mirhi_scope.h, mirhi_variant.h), as words; no HIP call.  in[0] says what is asked:
// 0  a scope: has_color, has_prim, has_depth, depth_is_array, depth_samples, depth_format, layers, depth_load_op, depth_store_op, view_mask, has_constants,
//    view_stride, view_offset (low, high word), the constants buffer's size (low, high word), area_partial, split_device, fragment_stats.
// 1  a draw's program: in[1].
// 2  the per-view plan: view_mask, layer width, layer height, view_offset (low, high), view_stride -> out: the number of view slots, then per slot five words:
//    view index, byte offset of its layer in the array (low, high), byte offset of its matrix in the view constants (low, high).
// 3  the raster launch of a 5 x 4 tile scope: zflip, zmask, tp_max_area, views -> msg: the kernel's name out of the launch table; out: family, keyed, tp, grid x, y, z,
//    block, batched_form, and the family value of the last older row (RASTER_MSAA).
// Returns 0 (accepted / answered; msg empty for 0 and 1), 1 (refused; msg: the words behind "Invalid handle: "), -1 for words it cannot take.
extern "C" int mirhi_debug_multiview(const uint32_t* in, uint32_t* out, char* msg, uint32_t msg_len) {
    const char* why = nullptr;
    auto u64 = [](uint32_t lo, uint32_t hi) { return (uint64_t)lo | (uint64_t)hi << 32; };
    if (in[0] == 0u) {
        MultiviewFacts f{};
        f.has_color = in[1]; f.has_prim = in[2]; f.has_depth = in[3]; f.depth_is_array = in[4]; f.depth_samples = in[5]; f.depth_format = in[6]; f.layers = in[7];
        f.depth_load_op = (int32_t)in[8]; f.depth_store_op = (int32_t)in[9]; f.view_mask = in[10]; f.has_constants = in[11]; f.view_stride = in[12];
        f.view_offset = u64(in[13], in[14]); f.constants_bytes = u64(in[15], in[16]); f.area_partial = in[17]; f.split_device = in[18]; f.fragment_stats = in[19];
        why = multiview_scope_refusal(f);
    } else if (in[0] == 1u) why = multiview_program_refusal((int32_t)in[1]);
    else if (in[0] == 2u) {
        MultiviewSlot slot[MAX_BATCH];
        const uint32_t n = multiview_slots(in[1], in[2], in[3], u64(in[4], in[5]), in[6], slot);
        out[0] = n;
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t words[5] = {slot[j].view, (uint32_t)slot[j].layer_offset, (uint32_t)(slot[j].layer_offset >> 32), (uint32_t)slot[j].matrix_offset, (uint32_t)(slot[j].matrix_offset >> 32)};
            memcpy(out + 1 + 5 * j, words, sizeof words);
        }
        if (msg && msg_len) msg[0] = 0;
        return 0;
    } else if (in[0] == 3u) {
        PassParams P{};
        P.tiles_x = 5u; P.tile_row_end = 4u; P.tile_row_step = 1u; P.zflip = in[1]; P.zmask = in[2]; P.tp_max_area = in[3]; P.depth_only = 1u;
        const RasterVariant v = multiview_variant(P, in[4]);
        const char* name = multiview_raster_name(v);
        const uint32_t words[9] = {(uint32_t)v.family, v.keyed, v.tp, v.grid[0], v.grid[1], v.grid[2], v.block, v.batched_form, (uint32_t)RASTER_MSAA};
        memcpy(out, words, sizeof words);
        snprintf(msg, msg_len, "%s", name ? name : "");
        return name ? 0 : -1;
    } else return -1;
    snprintf(msg, msg_len, "%s", why ? why : "");
    return why ? 1 : 0;
}

static mirhi_result timing_begin(mirhi_device* dev, uint32_t kernel, uint32_t lane, LaunchTiming* t) {
    hipEvent_t ev[2];
    for (hipEvent_t& e : ev) {
        if (!dev->free_events.empty()) { e = dev->free_events.back(); dev->free_events.pop_back(); }
        else HIP_TRY(hipEventCreate(&e));
    }
    t->start = ev[0]; t->stop = ev[1];
    dev->pending.push_back(TimedDispatch{ev[0], ev[1], kernel, lane});
    return MIRHI_OK;
}

// Attachments of a command buffer's recording that are still live images (dev->mu held).
template <typename F>
static void for_each_attachment(mirhi_device* dev, const mirhi_cmd* c, F&& f) {
    for (const RecordedPass& pass : c->planned) {
        // a layer view stands for its array: scopes that write layers and scopes that sample the array meet on one object (a live view's array is alive)
        for (mirhi_image* img : {pass.images.color, pass.images.depth, pass.images.prim_id})
            if (img && std::find(dev->images.begin(), dev->images.end(), img) != dev->images.end()) f(img->parent ? img->parent : img);
        // the shadow maps the scope samples count as attachments: a read after another lane's write (the shadow scope) and a write after another lane's
        // read (the next frame's shadow scope behind this frame's lit one) are both ordered
        for (mirhi_image* img : pass.sampled)
            if (img && std::find(dev->images.begin(), dev->images.end(), img) != dev->images.end()) f(img->parent ? img->parent : img);
    }
}
// `c` is about to run on `stream` (or, natively, on `nq`): anything that used one of its attachments last somewhere else, and is not known
// to have finished, goes first.  Between two HIP streams that is an event; with an AQL queue on either side the host waits (a frame loop
// never gets here: its fences have told the library that the earlier frame is done).
static mirhi_result order_attachments(mirhi_device* dev, mirhi_cmd* c, hipStream_t stream, NativeQueue* nq = nullptr) {
    hipError_t err = hipSuccess;
    for_each_attachment(dev, c, [&](mirhi_image* img) {
        const bool elsewhere = nq ? (img->last_native != nq && (img->last_native || img->last_stream)) : (img->last_native != nullptr || (img->last_stream && img->last_stream != stream));
        if (elsewhere && err == hipSuccess) {
            if (img->last_native) { if (!drain_native(dev, img->last_native)) err = hipErrorLaunchTimeOut; }
            else {
                bool live = false;
                for (hipStream_t st : dev->lanes) live |= st == img->last_stream;
                for (hipStream_t st : dev->aux_streams) live |= st == img->last_stream;       // (a band exchange wrote the image last)
                if (live && nq) err = hipStreamSynchronize(img->last_stream);
                else if (live) {
                    if (!dev->order_event) err = hipEventCreateWithFlags(&dev->order_event, hipEventDisableTiming);
                    if (err == hipSuccess) err = hipEventRecord(dev->order_event, img->last_stream);
                    if (err == hipSuccess) err = hipStreamWaitEvent(stream, dev->order_event, 0);
                }
            }
        }
        img->last_stream = nq ? nullptr : stream; img->last_native = nq; img->last_cmd = c; img->last_seq = c->submit_seq;
    });
    if (err == hipErrorLaunchTimeOut && dev->native && dev->native->lost.load(std::memory_order_acquire)) return device_lost(dev);
    if (err != hipSuccess) return hip_fail(err, "attachment ordering across queue lanes");
    return MIRHI_OK;
}
// submission `seq` of `c` has finished: its attachments need no ordering any more (unless something newer used them since)
static void release_attachments(mirhi_device* dev, const mirhi_cmd* c, uint64_t seq) {
    for_each_attachment(dev, c, [&](mirhi_image* img) { if (img->last_cmd == c && img->last_seq == seq) { img->last_stream = nullptr; img->last_native = nullptr; img->last_cmd = nullptr; } });
}

static mirhi_result submit_now(mirhi_device* dev, uint32_t cmd_count, mirhi_cmd* const* cmds, mirhi_fence* fence);

static void submit_thread_main(mirhi_device* dev) {
    (void)hipSetDevice(dev->ordinal);
    uint64_t taken = dev->sq_done.load(std::memory_order_acquire);      // (the thread may have been stopped and started again: the ring goes on where it was)
    for (;;) {
        uint32_t idle = 0;
        while (dev->sq_pushed.load(std::memory_order_acquire) == taken) {
            if (dev->sq_stop.load(std::memory_order_acquire)) return;
            cpu_relax();
            if (++idle > 40000u) {                    // ~100 us without work: sleep until the next submit
                std::unique_lock<std::mutex> lk(dev->sq_mu);
                dev->sq_sleeping.store(true, std::memory_order_seq_cst);
                dev->sq_cv.wait(lk, [&] { return dev->sq_pushed.load(std::memory_order_acquire) != taken || dev->sq_stop.load(std::memory_order_acquire); });
                dev->sq_sleeping.store(false, std::memory_order_seq_cst);
                idle = 0;
            }
        }
        mirhi_device::SubmitJob& job = dev->sq_ring[taken % mirhi_device::SQ_SLOTS];
        const mirhi_result rc = submit_now(dev, job.n, job.cmds, job.fence);
        if (rc != MIRHI_OK) {
            // the caller returned long ago: the failure is reported where the submission's completion is asked for
            std::lock_guard<std::mutex> lock(dev->mu);
            if (job.fence) { job.fence->deferred = rc; job.fence->deferred_msg = g_last_error; job.fence->pending = true; }
            else { dev->deferred = rc; dev->deferred_msg = g_last_error; }
        }
        if (job.fence) job.fence->issued.store(true, std::memory_order_release);
        for (uint32_t i = 0; i < job.n; i++) job.cmds[i]->queued.fetch_sub(1, std::memory_order_release);
        taken++;
        dev->sq_done.store(taken, std::memory_order_release);
    }
}

extern "C" mirhi_result mirhi_device_set_submit_thread(mirhi_device* dev, uint32_t enable) {
    NULL_CHECK(dev, "device");
    if ((enable != 0) == dev->sq_on) return MIRHI_OK;
    if (enable) {
        dev->sq_stop.store(false);
        try { dev->sq_thread = std::thread(submit_thread_main, dev); }
        catch (...) { return fail(MIRHI_ERR_DEVICE, "Vulkan error: could not start the submit thread"); }
        dev->sq_on = true;
    } else {
        drain_submits(dev);
        { std::lock_guard<std::mutex> lk(dev->sq_mu); dev->sq_stop.store(true); }
        dev->sq_cv.notify_all();
        if (dev->sq_thread.joinable()) dev->sq_thread.join();
        dev->sq_on = false;
    }
    return MIRHI_OK;
}

extern "C" mirhi_result mirhi_queue_submit(mirhi_device* dev, uint32_t cmd_count, mirhi_cmd* const* cmds, mirhi_fence* fence) {
    NULL_CHECK(dev, "device");
    if (cmd_count) NULL_CHECK(cmds, "cmds");
    for (uint32_t i = 0; i < cmd_count; i++) {
        NULL_CHECK(cmds[i], "cmds[i]");
        if (cmds[i]->dev != dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: command buffer belongs to another device");
        if (cmds[i]->state != CMD_EXECUTABLE) return fail(MIRHI_ERR_DEVICE, "Vulkan error: command buffer %u is not in the executable state (call end())", i);
    }
    if (fence && fence->dev != dev) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: fence belongs to another device");
    // a lost device refuses a submit here, in the caller's thread, whether or not a submit thread would have issued it (vkQueueSubmit: VK_ERROR_DEVICE_LOST)
    if (dev->native && dev->native->lost.load(std::memory_order_acquire)) return device_lost(dev);
    constexpr uint32_t JOB_CMDS = sizeof(mirhi_device::SubmitJob::cmds) / sizeof(mirhi_cmd*);
    if (!dev->sq_on || cmd_count > JOB_CMDS) {
        drain_submits(dev);
        return submit_now(dev, cmd_count, cmds, fence);
    }
    // Submit thread on: the job is queued, the launches happen there.  What the caller may look at next is set here, in its own thread.
    std::lock_guard<std::mutex> producer(dev->sq_push_mu);
    const uint64_t slot = dev->sq_pushed.load(std::memory_order_relaxed);
    while (slot - dev->sq_done.load(std::memory_order_acquire) >= mirhi_device::SQ_SLOTS) cpu_relax();
    mirhi_device::SubmitJob& job = dev->sq_ring[slot % mirhi_device::SQ_SLOTS];
    job.n = cmd_count; job.fence = fence;
    for (uint32_t i = 0; i < cmd_count; i++) { job.cmds[i] = cmds[i]; cmds[i]->queued.fetch_add(1, std::memory_order_relaxed); }
    if (fence) { fence->issued.store(false, std::memory_order_relaxed); fence->pending = true; fence->signaled = false; }
    dev->sq_pushed.store(slot + 1, std::memory_order_seq_cst);
    if (dev->sq_sleeping.load(std::memory_order_seq_cst)) { std::lock_guard<std::mutex> lk(dev->sq_mu); dev->sq_cv.notify_one(); }
    return MIRHI_OK;
}

// What the steps of one submit share.  dev->mu guards the bookkeeping (unchecked list, statistics, attachment ordering, timed-dispatch events), not
// the launches: with the submit thread on, the render thread must be able to complete a fence while this thread is inside hipLaunchKernel -- a
// step lets go of the lock around its launches (unlock / relock) unless keep_locked.
struct Submit {
    mirhi_device* dev;
    std::unique_lock<std::mutex> lock;
    bool keep_locked;
    SubmitDevice device;              // the facts a submit looks at, in the device, the switches ...
    SubmitSwitches sw;
    SubmitPath path;                  // ... and the command buffers: the path they give (mirhi_submit.h: every "whether" of a submit is decided there)
    NativeQueue* nq;                  // the lane's AQL queue, when the submit goes out as packets
    mirhi_fence* fence;
    FenceCarrier carrier;
    void unlock() { if (!keep_locked) lock.unlock(); }
    void relock() { if (!keep_locked) lock.lock(); }
};

static hipStream_t lane_stream(const mirhi_device* dev, uint32_t lane) { return dev->lanes[lane < dev->lanes.size() ? lane : 0]; }

// The fence's signal or event, made on first use, and what of the submit will signal it
static mirhi_result prepare_fence(Submit& s) {
    mirhi_fence* fence = s.fence;
    s.carrier = fence_carrier(s.path, s.device, s.sw, fence != nullptr);
    if (fence && s.nq) {
        fence->native_q = s.nq;
        if (!fence->native_sig.handle && hsa_signal_create(0, 0, nullptr, &fence->native_sig) != HSA_STATUS_SUCCESS) return fail(MIRHI_ERR_DEVICE, "Vulkan error: hsa_signal_create for a fence failed");
        hsa_signal_store_relaxed(fence->native_sig, 1);
    }
    if (fence && !s.nq && !fence->event) HIP_TRY(hipEventCreate(&fence->event));
    return MIRHI_OK;
}

// `c` is about to run on `stream` (or, natively, on `nq`): wherever else it ran last is drained (its workspace may still be in use there), it is
// pending on its new place as submission submit_seq, and its attachments are ordered behind their last users
static mirhi_result claim_cmd(mirhi_device* dev, mirhi_cmd* c, hipStream_t stream, NativeQueue* nq) {
    if (c->pending && c->last_native && c->last_native != nq && !drain_native(dev, c->last_native)) return device_lost(dev);      // (last_native or last_stream: never both)
    if (c->pending && c->last_stream && (nq || c->last_stream != stream)) HIP_TRY(hipStreamSynchronize(c->last_stream));
    c->last_stream = nq ? nullptr : stream; c->last_native = nq; c->pending = true; c->submit_seq++;
    { const mirhi_result ro = order_attachments(dev, c, stream, nq); if (ro != MIRHI_OK) return ro; }
    if (std::find(dev->unchecked.begin(), dev->unchecked.end(), c) == dev->unchecked.end()) dev->unchecked.push_back(c);
    return MIRHI_OK;
}

// the batched launch triple on the first command buffer's lane
static mirhi_result issue_batch(Submit& s, uint32_t cmd_count, mirhi_cmd* const* cmds) {
    mirhi_device* dev = s.dev;
    hipStream_t stream = lane_stream(dev, cmds[0]->lane);
    const PassParams* P[MAX_BATCH]; const PassParams* dp[MAX_BATCH]; uint32_t* big[MAX_BATCH];
    for (uint32_t i = 0; i < cmd_count; i++) {
        mirhi_cmd* c = cmds[i];
        { const mirhi_result rc = claim_cmd(dev, c, stream, nullptr); if (rc != MIRHI_OK) return rc; }
        P[i] = &c->plan[0];
        const uint32_t parity = c->ws.scope_bins.take_parity(0);
        dp[i] = c->ws.params + parity;
        big[i] = c->ws.scope_bins.slot(0).counters + CTR_BIG + parity;
        dev->stats.frames_submitted++;
        dev->stats.triangles_submitted += c->plan[0].total_tris;
    }
    s.unlock();
    hipError_t le = launch_vertex_batch(P, dp, cmd_count, stream);
    if (le == hipSuccess) le = launch_geometry_batch(P, dp, cmd_count, stream);
    if (le == hipSuccess) le = launch_raster_batch(P, dp, big, cmd_count, cmds[0]->plan_programs[0], stream, s.carrier == FENCE_STOP_EVENT ? s.fence->event : nullptr);
    s.relock();
    HIP_TRY(le);
    return MIRHI_OK;
}

// One scope of command buffer `c`: its vertex, geometry and raster launch (with_fence: the raster launch carries the submit's fence), and with
// profiling on their timing events and the statistics pass
// A multiview depth scope: the views of scope `pi` as ONE vertex, ONE geometry and ONE raster launch, on either dispatch path.  CLEAR and LOAD
// alike: a view loads, tests and stores its own layer and nothing else, so no view depends on another.  Every view slot works on its own slice of the workspace
// with its own big-list parity; the single-view buffers and their parity are left alone.
static mirhi_result issue_multiview(Submit& s, mirhi_cmd* c, size_t pi, hipStream_t stream, bool with_fence) {
    mirhi_device* dev = s.dev;
    const mirhi_cmd::ViewSet& vs = c->plan_views[pi];
    Workspace& w = c->ws;
    const PassParams* hp[MAX_BATCH]; const PassParams* dp[MAX_BATCH]; uint32_t* big[MAX_BATCH];
    for (uint32_t j = 0; j < vs.count; j++) {
        const uint32_t parity = w.view_bins.take_parity(j);
        hp[j] = &c->plan_view_params[vs.first + j];
        dp[j] = reinterpret_cast<const PassParams*>(w.pblock + w.layout.slot_params(vs.first + j, parity));
        big[j] = w.view_bins.slot(j).counters + CTR_BIG + parity;
    }
    const PassParams& P = *hp[0];
    LaunchTiming tv{}, tg{}, tr{};
    if (s.nq) {
        const uint64_t foreign = dev->foreign_writes.load(std::memory_order_acquire);
        const PacketScopes scopes = packet_scopes(P, s.sw.system_scope, s.nq->seen_foreign != foreign, w.foreign);
        s.nq->seen_foreign = foreign; w.foreign = false;
        tv.native = s.nq; tg.native = s.nq; tr.native = s.nq;
        tv.native_flags = scopes.vertex; tg.native_flags = scopes.geometry; tr.native_flags = scopes.raster;
    }
    tg.tris_per_wave = tris_per_wave(P, s.sw.geom_tpw);
    if (scope_timed(dev->profiling, c->lane)) {
        mirhi_result r;
        if (P.vs_total_slots && (r = timing_begin(dev, MIRHI_KERNEL_VERTEX, c->lane, &tv)) != MIRHI_OK) return r;
        if (P.total_slots && (r = timing_begin(dev, MIRHI_KERNEL_GEOMETRY, c->lane, &tg)) != MIRHI_OK) return r;
        if (has_tiles(P) && (r = timing_begin(dev, MIRHI_KERNEL_RASTER, c->lane, &tr)) != MIRHI_OK) return r;
    }
    if (with_fence && s.carrier == FENCE_STOP_EVENT) tr.stop = s.fence->event;
    if (with_fence && s.carrier == FENCE_NATIVE_SIGNAL) tr.native_signal = s.fence->native_sig.handle;
    s.unlock();
    hipError_t le = launch_multiview_vertex(hp, dp, vs.count, stream, tv);
    if (le == hipSuccess) le = launch_multiview_geometry(hp, dp, vs.count, stream, tg);
    if (le == hipSuccess) le = launch_multiview_raster(hp, dp, big, vs.count, stream, tr);
    s.relock();
    HIP_TRY(le);
    dev->stats.frames_submitted++;
    dev->stats.triangles_submitted += (uint64_t)P.total_tris * vs.count;
    return MIRHI_OK;
}

static mirhi_result issue_scope(Submit& s, mirhi_cmd* c, size_t pi, hipStream_t stream, bool wide_allowed, bool with_fence) {
    if (pi < c->plan_views.size() && c->plan_views[pi].count) return issue_multiview(s, c, pi, stream, with_fence);
    mirhi_device* dev = s.dev;
    const PassParams& P = c->plan[pi];
    // alternate the big-list counter: the raster kernel zeroes the other one for the next scope
    BinSet& bins = c->ws.scope_bins;
    const uint32_t parity = flips_parity(P) ? bins.take_parity(0) : bins.parity_of(0);
    const PassParams* dp = reinterpret_cast<const PassParams*>(c->ws.pblock + BlockLayout::scope_params(pi, parity));
    uint32_t* big_count = bins.slot(0).counters + CTR_BIG + parity;
    // ordered segment: slots of primitives that no draw of the segment covers (a Never draw keeps its ids) must read
    // as "no coverage" -- an all-zero record is a degenerate triangle whose edge functions are negative everywhere
    if (P.ordered_recs && P.ordered_count) HIP_TRY(hipMemsetAsync(P.ordered_recs, 0, (size_t)P.ordered_count * sizeof(TriRec), stream));
    LaunchTiming tv{}, tg{}, tc{}, tr{};
    if (s.nq) {
        const uint64_t foreign = dev->foreign_writes.load(std::memory_order_acquire);
        const PacketScopes scopes = packet_scopes(P, s.sw.system_scope, s.nq->seen_foreign != foreign, c->ws.foreign);
        s.nq->seen_foreign = foreign; c->ws.foreign = false;
        tv.native = s.nq; tg.native = s.nq; tr.native = s.nq;
        tv.native_flags = scopes.vertex; tg.native_flags = scopes.geometry; tr.native_flags = scopes.raster;
    }
    tg.tris_per_wave = tris_per_wave(P, s.sw.geom_tpw);
    if (pi < c->planned.size() && c->planned[pi].draws.size() == 1u) tg.head_draw = &c->planned[pi].draws[0];      // (GeometryHead::vb0: launch_geometry decides)
    const bool timed = scope_timed(dev->profiling, c->lane);
    if (timed) {
        mirhi_result r;
        if (P.vs_total_slots && (r = timing_begin(dev, MIRHI_KERNEL_VERTEX, c->lane, &tv)) != MIRHI_OK) return r;
        if (P.total_slots && (r = timing_begin(dev, MIRHI_KERNEL_GEOMETRY, c->lane, &tg)) != MIRHI_OK) return r;
    }
    s.unlock();
    hipError_t le = launch_vertex(P, dp, stream, tv);
    if (le == hipSuccess) le = launch_geometry(P, dp, stream, tg);
    s.relock();
    HIP_TRY(le);
    const uint32_t* winners = nullptr;
    if (scope_counted(dev->profiling, P)) {
        mirhi_result r;
        if (timed && (r = timing_begin(dev, MIRHI_KERNEL_FRAGMENT_COUNT, c->lane, &tc)) != MIRHI_OK) return r;
        HIP_TRY(launch_fragment_count(P, dp, big_count, stream, tc));
        dev->frag_scopes++;
        // winners are counted from a primitive-id image: the scope's own if every pixel of it is written (no LOAD),
        // else the workspace's, cleared to NO_PRIM, through a copy of the parameters -- the raster kernels know nothing
        // of the statistics
        // (a partial render area leaves the pixels outside it as they were: not every pixel is written then either)
        if (P.prim_out && !P.color_load && !P.area_partial) winners = P.prim_out;
        else {
            if ((r = stats_params_for(c)) != MIRHI_OK) return r;
            HIP_TRY(hipMemsetAsync(c->ws.stats_prim, 0xFF, (size_t)P.width * P.height * 4, stream));
            dp = c->ws.stats_params + (dp - c->ws.params);
            winners = c->ws.stats_prim;
        }
    }
    if (timed && has_tiles(P)) { mirhi_result r = timing_begin(dev, MIRHI_KERNEL_RASTER, c->lane, &tr); if (r != MIRHI_OK) return r; }
    if (with_fence && s.carrier == FENCE_STOP_EVENT) tr.stop = s.fence->event;
    if (with_fence && s.carrier == FENCE_NATIVE_SIGNAL) tr.native_signal = s.fence->native_sig.handle;
    s.unlock();
    le = launch_raster(P, dp, big_count, c->plan_programs[pi], stream, tr, wide_allowed);
    s.relock();
    HIP_TRY(le);
    if (winners) HIP_TRY(launch_winner_count(winners, P.width * P.height, dev->frag_stats, stream));
    if (!P.xfer) dev->stats.frames_submitted++;      // (a transfer is no rendering scope)
    dev->stats.triangles_submitted += P.total_tris;
    return MIRHI_OK;
}

// Nothing of the submit carried the fence
static mirhi_result attach_fence(Submit& s, uint32_t cmd_count, mirhi_cmd* const* cmds) {
    mirhi_fence* fence = s.fence;
    if (s.carrier == FENCE_NATIVE_DRAIN) {            // (no tiles to raster): wait here, the fence is signalled at once
        native_queue_drain(s.nq);
        hsa_signal_store_relaxed(fence->native_sig, 0);
    }
    if (s.carrier == FENCE_EVENT_RECORD) {
        // the fence follows the last command buffer's lane and waits for the other lanes used by this submit
        hipStream_t fstream = cmd_count ? cmds[cmd_count - 1]->last_stream : s.dev->stream;
        for (uint32_t i = 0; i + 1 < cmd_count; i++) {
            hipStream_t other = cmds[i]->last_stream;
            if (other != fstream) {
                if (!fence->join) HIP_TRY(hipEventCreateWithFlags(&fence->join, hipEventDisableTiming));
                HIP_TRY(hipEventRecord(fence->join, other));
                HIP_TRY(hipStreamWaitEvent(fstream, fence->join, 0));
            }
        }
        HIP_TRY(hipEventRecord(fence->event, fstream));
    }
    return MIRHI_OK;
}

static mirhi_result submit_now(mirhi_device* dev, uint32_t cmd_count, mirhi_cmd* const* cmds, mirhi_fence* fence) {
    HIP_TRY(hipSetDevice(dev->ordinal));
    const PlanKnobs knobs = PlanKnobs::read();
    // 1. replan where an earlier submission ran out of bin pages (a bigger pool, the same plan) or showed a spread-out mesh (one team)
    for (uint32_t i = 0; i < cmd_count; i++)
        if ((cmds[i]->ws.grow_pool && !knobs.pool_pages.set) || cmds[i]->ws.replan) {
            const mirhi_result rp = build_plan(cmds[i], true);
            if (rp != MIRHI_OK) return rp;
        }
    // 2. the facts, and the path they give
    const NativeEnv& env = native_env();
    Submit s{dev, std::unique_lock<std::mutex>(dev->mu), dev->profiling != 0,
             SubmitDevice{dev->profiling, dev->native && dev->native->ok, dev->owns_stream, dev->native_on_external, (uint32_t)dev->lanes.size()},
             SubmitSwitches{env.no_batch, env.fence_record, env.system_scope, env.geom_tpw, knobs.raster_wide.set}, SubmitPath{}, nullptr, fence, FENCE_NONE};
    s.path = submit_path(s.device, s.sw, cmd_count, [&](uint32_t i) { return submit_cmd(cmds[i], cmds[i]->lane, cmds[i]->plan.data(), cmds[i]->plan.size()); },
                         [&](uint32_t i) { return submit_head(cmds[i]->plan[0], cmds[i]->plan_programs[0]); });
    s.nq = s.path.native ? native_lane(dev, cmds[0]->lane) : nullptr;
    s.path.native = s.nq != nullptr;
    if (s.nq) s.keep_locked = true;       // (an AQL queue has one producer at a time, and a dispatch takes 0.2 us: the device lock stays held)
    if (fence) fence->native_wait = false;
    if (s.nq && dev->native->lost.load(std::memory_order_acquire)) return device_lost(dev);
    // 3. the fence
    { const mirhi_result rf = prepare_fence(s); if (rf != MIRHI_OK) return rf; }
    // 4. claim and issue: one batch, or command buffer by command buffer, scope by scope
    if (s.path.batched) { const mirhi_result rb = issue_batch(s, cmd_count, cmds); if (rb != MIRHI_OK) return rb; }
    for (uint32_t i = 0; !s.path.batched && i < cmd_count; i++) {
        mirhi_cmd* c = cmds[i];
        hipStream_t stream = lane_stream(dev, c->lane);
        { const mirhi_result rc = claim_cmd(dev, c, stream, s.nq); if (rc != MIRHI_OK) return rc; }
        int in_flight = 1;
        for (const mirhi_cmd* o : dev->cmds) in_flight += (o != c && o->pending) ? 1 : 0;
        const bool wide_allowed = allow_wide(in_flight, s.sw.wide_set);
        for (size_t pi = 0; pi < c->plan.size(); pi++) {
            const mirhi_result rs = issue_scope(s, c, pi, stream, wide_allowed, carries_fence(s.carrier, s.path, i, pi));
            if (rs != MIRHI_OK) return rs;
        }
    }
    // 5. the fence, if nothing carried it
    { const mirhi_result ra = attach_fence(s, cmd_count, cmds); if (ra != MIRHI_OK) return ra; }
    // 6. bookkeeping
    if (fence) {
        if (s.nq) fence->native_wait = true;
        fence->pending = true; fence->signaled = false;
        fence->cmds.assign(cmds, cmds + cmd_count);
        fence->seqs.resize(cmd_count);
        for (uint32_t i = 0; i < cmd_count; i++) fence->seqs[i] = cmds[i]->submit_seq;
        fence->deferred = MIRHI_OK; fence->deferred_msg.clear();
    }
    return MIRHI_OK;
}

extern "C" mirhi_result mirhi_fence_create(mirhi_device* dev, uint32_t signaled, mirhi_fence** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    mirhi_fence* f = new (std::nothrow) mirhi_fence();
    if (!f) return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed");
    f->dev = dev; f->signaled = signaled != 0;
    { std::lock_guard<std::mutex> lock(dev->mu); dev->fences.push_back(f); }
    dev->children++;
    *out = f;
    return MIRHI_OK;
}
// device-side status of one finished command buffer -> stats + error (the same text whether a fence or wait_idle finds it)
static mirhi_result status_of(mirhi_device* dev, mirhi_cmd* c) {
    mirhi_result r = MIRHI_OK;
    if (c->ws.status_host) {
        // (the view slots of a multiview scope report in words of their own behind the scopes': their bits count like a scope's, their big lists by the longest)
        const uint32_t bits = c->ws.status_bits();
        uint32_t big_list = c->ws.status_host[1];
        for (uint32_t j = 0; j < (uint32_t)MAX_BATCH; j++) big_list = std::max(big_list, c->ws.status_host[Workspace::STATUS_VIEWS + 4u * j + 1u]);
        dev->stats.last_status = bits;
        dev->stats.last_big_list = big_list;
        dev->stats.last_bin_pages = c->ws.status_host[2];
        // (the plan feedback below rewrites flags build_plan reads: not while the submit thread may be re-planning a queued submission of this command
        // buffer -- the status words stay set and the next look at them, with nothing queued, acts on them)
        const bool feedback = c->queued.load(std::memory_order_acquire) == 0;
        if (feedback && (bits & STATUS_POOL_EXHAUSTED) && !c->ws.grow_pool) {
            // not an error: the records went to the big list and the frame is complete; the pool is doubled in front of the next submit
            c->ws.grow_pool = true;
            if (c->ws.pool_scale < 64u) c->ws.pool_scale *= 2u;
        }
        if (feedback && (c->ws.status_host[3] & 0x80000000u)) {
            // busy tiles of the scope before this one: few of them = a mesh in a part of the frame = the wide variant (and back), see Workspace::wide
            c->ws.busy_tiles = c->ws.status_host[3] & 0x7FFFFFFFu; c->ws.busy_known = true;
            const uint32_t cur = c->ws.wide, want = wide_wanted(c->ws.busy_tiles, cur);
            if (want != cur && c->ws.wide_eligible && !PlanKnobs::read().raster_wide.set) { c->ws.wide = want; c->ws.replan = true; }
        }
        if (feedback && !c->ws.spread && c->ws.xcd_tiles_last && c->ws.status_host[2] > 2u * c->ws.xcd_tiles_last) { c->ws.spread = true; c->ws.replan = true; c->ws.spread_tris = c->plan_tris; }
        if (bits & (STATUS_PAGE_TIMEOUT | STATUS_BIG_OVERFLOW)) c->ws.scope_bins.dirty = true;    // counters / page table are cleared before the next frame
        if (bits & STATUS_PAGE_TIMEOUT)
            r = fail(MIRHI_ERR_DEVICE, "Vulkan error: rasterizer bin page was never published; frame is incomplete");
        if (bits & STATUS_ALPHA_TEST_TEXTURED)
            r = fail(MIRHI_ERR_PIPELINE, "Pipeline error: MODEL_PBR alpha cutoff together with a base colour texture needs a per-fragment discard: set mirhi_pipeline_desc.fragment_discard_enable on that pipeline; the draw was skipped");
        if (bits & STATUS_BIG_OVERFLOW)
            r = fail(MIRHI_ERR_DEVICE, "Vulkan error: rasterizer large-triangle list overflowed (%u entries); frame is incomplete", big_list);
    }
    return r;
}
static mirhi_result check_status_words(mirhi_device* dev) {
    std::lock_guard<std::mutex> lock(dev->mu);
    mirhi_result r = MIRHI_OK;
    for (mirhi_cmd* c : dev->unchecked) { const mirhi_result rc = status_of(dev, c); if (rc != MIRHI_OK) r = rc; }
    dev->unchecked.clear();
    for (mirhi_cmd* c : dev->cmds) cmd_finished(c);       // (called with every lane synchronised)
    for (mirhi_image* img : dev->images) { img->last_stream = nullptr; img->last_native = nullptr; img->last_cmd = nullptr; }
    if (dev->deferred != MIRHI_OK) { if (r == MIRHI_OK) { r = dev->deferred; g_last_error = dev->deferred_msg; } dev->deferred = MIRHI_OK; dev->deferred_msg.clear(); }
    return r;
}
static mirhi_result fence_complete(mirhi_fence* f) {
    f->pending = false; f->signaled = true;
    mirhi_result r = MIRHI_OK;
    {
        std::lock_guard<std::mutex> lock(f->dev->mu);          // what a fence has reported is not reported again by wait_idle
        for (size_t i = 0; i < f->cmds.size(); i++) {
            mirhi_cmd* c = f->cmds[i];
            const mirhi_result rc = status_of(f->dev, c); if (rc != MIRHI_OK) r = rc;
            release_attachments(f->dev, c, f->seqs[i]);
            if (c->submit_seq == f->seqs[i]) {              // (a later submission of the same command buffer is still its own fence's business)
                cmd_finished(c);
                auto& u = f->dev->unchecked;
                u.erase(std::remove(u.begin(), u.end(), c), u.end());
            }
        }
    }
    f->cmds.clear(); f->seqs.clear();
    if (f->deferred != MIRHI_OK) { if (r == MIRHI_OK) { r = f->deferred; g_last_error = f->deferred_msg; } f->deferred = MIRHI_OK; f->deferred_msg.clear(); }
    return r;
}
extern "C" mirhi_result mirhi_fence_wait(mirhi_fence* f, uint64_t timeout_ns) {
    NULL_CHECK(f, "fence");
    if (f->signaled) return MIRHI_OK;
    if (f->pending && !f->issued.load(std::memory_order_acquire)) {
        // its submission still waits in the submit thread's queue (microseconds): the event is recorded when it is issued
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::nanoseconds(timeout_ns < 4000000000ull ? timeout_ns : 4000000000ull);
        for (uint32_t it = 0; !f->issued.load(std::memory_order_acquire); it++) {
            cpu_relax();
            if (timeout_ns != UINT64_MAX && (it & 255u) == 255u && std::chrono::steady_clock::now() >= deadline) return fail(MIRHI_TIMEOUT, "Vulkan error: TIMEOUT");
        }
    }
    if (!f->pending) {
        // unsignaled and nothing submitted: Vulkan would block until the timeout
        if (timeout_ns == UINT64_MAX) return fail(MIRHI_ERR_DEVICE, "Vulkan error: waiting forever on a fence that was never submitted");
        std::this_thread::sleep_for(std::chrono::nanoseconds(timeout_ns < 1000000000ull ? timeout_ns : 1000000000ull));
        return fail(MIRHI_TIMEOUT, "Vulkan error: TIMEOUT");
    }
    if (f->native_wait) {
        // native dispatch: the completion signal of the submission's last packet, a word in host memory (1 -> 0).  Bounded whatever the caller's timeout:
        // a queue that stops making progress for the device's deadline is a lost device (VK_ERROR_DEVICE_LOST), not a thread that spins forever.
        const int w = native_signal_wait(f->native_sig, timeout_ns, f->dev->native, f->native_q, "waiting for a fence");
        if (w == 1) return fail(MIRHI_TIMEOUT, "Vulkan error: TIMEOUT");
        if (w == 2) return device_lost(f->dev);
        f->native_wait = false;
        return fence_complete(f);
    }
    if (!f->event) {
        // nothing was ever recorded for this submission: it failed in the submit thread before its first launch (the error is the deferred one)
        f->pending = false;
        if (f->deferred != MIRHI_OK) { const mirhi_result r = f->deferred; g_last_error = f->deferred_msg; f->deferred = MIRHI_OK; f->deferred_msg.clear(); f->cmds.clear(); f->seqs.clear(); return r; }
        return fail(MIRHI_ERR_DEVICE, "Vulkan error: fence has no submission to wait for");
    }
    HIP_TRY(hipSetDevice(f->dev->ordinal));
    if (timeout_ns == UINT64_MAX) {
        // a frame loop's fence is due within microseconds: poll (60 ns per query) for a while before blocking in the runtime
        const auto spin_until = std::chrono::steady_clock::now() + std::chrono::microseconds(200);
        for (uint32_t it = 0;; it++) {
            hipError_t e = hipEventQuery(f->event);
            if (e == hipSuccess) return fence_complete(f);
            if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery");
            (void)hipGetLastError();
            // (a query takes the runtime's locks: back to back from this thread it starves the thread that is launching)
            for (int k = 0; k < 16; k++) cpu_relax();
            if ((it & 63u) == 63u && std::chrono::steady_clock::now() >= spin_until) break;
        }
        HIP_TRY(hipEventSynchronize(f->event));
        return fence_complete(f);
    }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::nanoseconds(timeout_ns);
    for (;;) {
        hipError_t e = hipEventQuery(f->event);
        if (e == hipSuccess) return fence_complete(f);
        if (e != hipErrorNotReady) return hip_fail(e, "hipEventQuery");
        (void)hipGetLastError();
        if (std::chrono::steady_clock::now() >= deadline) return fail(MIRHI_TIMEOUT, "Vulkan error: TIMEOUT");
        std::this_thread::yield();
    }
}
extern "C" mirhi_result mirhi_fence_reset(mirhi_fence* f) {
    NULL_CHECK(f, "fence");
    if (f->pending) {   // resetting a fence that is still in flight is invalid in Vulkan; drain it first
        while (!f->issued.load(std::memory_order_acquire)) cpu_relax();
        HIP_TRY(hipSetDevice(f->dev->ordinal));
        if (f->native_wait) { (void)native_signal_wait(f->native_sig, UINT64_MAX, f->dev->native, f->native_q, "resetting a pending fence"); f->native_wait = false; }
        else if (f->event) HIP_TRY(hipEventSynchronize(f->event));
        (void)fence_complete(f);
    }
    f->signaled = false;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_fence_status(mirhi_fence* f) {
    NULL_CHECK(f, "fence");
    if (f->signaled) return MIRHI_OK;
    if (!f->pending || !f->issued.load(std::memory_order_acquire)) return MIRHI_NOT_READY;
    if (f->native_wait) {
        if (hsa_signal_load_scacquire(f->native_sig) != 0) return MIRHI_NOT_READY;
        f->native_wait = false; (void)fence_complete(f);
        return MIRHI_OK;
    }
    if (!f->event) return MIRHI_NOT_READY;        // (a submission that failed in the submit thread: mirhi_fence_wait reports it)
    (void)hipSetDevice(f->dev->ordinal);
    hipError_t e = hipEventQuery(f->event);
    if (e == hipSuccess) { (void)fence_complete(f); return MIRHI_OK; }
    (void)hipGetLastError();
    return MIRHI_NOT_READY;
}
extern "C" mirhi_result mirhi_fence_destroy(mirhi_fence* f) {
    NULL_CHECK(f, "fence");
    (void)hipSetDevice(f->dev->ordinal);
    while (!f->issued.load(std::memory_order_acquire)) cpu_relax();
    if (f->pending && f->native_wait) (void)native_signal_wait(f->native_sig, UINT64_MAX, f->dev->native, f->native_q, "destroying a pending fence");
    else if (f->pending && f->event) (void)hipEventSynchronize(f->event);
    if (f->native_sig.handle) (void)hsa_signal_destroy(f->native_sig);
    if (f->event) (void)hipEventDestroy(f->event);
    if (f->join) (void)hipEventDestroy(f->join);
    { std::lock_guard<std::mutex> lock(f->dev->mu); auto& v = f->dev->fences; v.erase(std::remove(v.begin(), v.end(), f), v.end()); }
    f->dev->children--;
    delete f;
    return MIRHI_OK;
}

// ------------------------------------------------------------------------------------------------
// measurement
// ------------------------------------------------------------------------------------------------
extern "C" mirhi_result mirhi_device_set_profiling(mirhi_device* dev, uint32_t enable) {
    NULL_CHECK(dev, "device");
    drain_submits(dev);
    std::lock_guard<std::mutex> lock(dev->mu);
    dev->profiling = enable & (MIRHI_PROFILE_TIMING | MIRHI_PROFILE_FRAGMENTS | 0xFF00u);
    return MIRHI_OK;
}
// Reads the timed dispatches back: duration = elapsed(start, stop) of the dispatch's own pair; position on the timeline =
// distance of its end from the end of the first dispatch since the last reset (hipEventElapsedTime between the stop events of
// two dispatches is the difference of their completion timestamps, whichever streams they ran on).
static mirhi_result drain_events(mirhi_device* dev) {
    HIP_TRY(hipSetDevice(dev->ordinal));
    for (TimedDispatch& p : dev->pending) {
        HIP_TRY(hipEventSynchronize(p.stop));
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, p.start, p.stop));
        bool keep_stop = false;
        double end_ms;
        if (!dev->base_stop) { dev->base_stop = p.stop; dev->base_end_ms = ms; end_ms = ms; keep_stop = true; }
        else { float rel = 0.0f; HIP_TRY(hipEventElapsedTime(&rel, dev->base_stop, p.stop)); end_ms = dev->base_end_ms + rel; }
        if (p.kernel < MIRHI_KERNEL_COUNT) { dev->total_ms[p.kernel] += ms; dev->launches[p.kernel]++; }
        if (dev->timeline.size() < (1u << 20)) dev->timeline.push_back(mirhi_dispatch_time{p.kernel, p.lane, (end_ms - ms) * 1e3, end_ms * 1e3});
        dev->free_events.push_back(p.start);
        if (!keep_stop) dev->free_events.push_back(p.stop);
    }
    dev->pending.clear();
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_kernel_time(mirhi_device* dev, mirhi_kernel_id kernel, double* total_ms, uint64_t* launches) {
    NULL_CHECK(dev, "device");
    if ((int)kernel < 0 || (int)kernel >= MIRHI_KERNEL_COUNT) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown kernel id %d", (int)kernel);
    drain_submits(dev);
    std::lock_guard<std::mutex> lock(dev->mu);
    mirhi_result r = drain_events(dev);
    if (r != MIRHI_OK) return r;
    if (total_ms) *total_ms = dev->total_ms[kernel];
    if (launches) *launches = dev->launches[kernel];
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_timeline(mirhi_device* dev, mirhi_dispatch_time* out, uint32_t capacity, uint32_t* count) {
    NULL_CHECK(dev, "device"); NULL_CHECK(count, "count");
    drain_submits(dev);
    std::lock_guard<std::mutex> lock(dev->mu);
    mirhi_result r = drain_events(dev);
    if (r != MIRHI_OK) return r;
    *count = (uint32_t)dev->timeline.size();
    if (out) for (uint32_t i = 0; i < capacity && i < *count; i++) out[i] = dev->timeline[i];
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_fragment_stats(mirhi_device* dev, uint64_t* shaded_pixels, uint64_t* covered_fragments, uint64_t* scopes) {
    NULL_CHECK(dev, "device");
    { mirhi_result r0 = sync_all_lanes(dev); if (r0 != MIRHI_OK) return r0; }
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, dev->frag_stats, sizeof v, hipMemcpyDeviceToHost, dev->stream));
    HIP_TRY(hipStreamSynchronize(dev->stream));
    if (shaded_pixels) *shaded_pixels = v[0];
    if (covered_fragments) *covered_fragments = v[1];
    if (scopes) { std::lock_guard<std::mutex> lock(dev->mu); *scopes = dev->frag_scopes; }
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_reset_kernel_times(mirhi_device* dev) {
    NULL_CHECK(dev, "device");
    { mirhi_result r0 = sync_all_lanes(dev); if (r0 != MIRHI_OK) return r0; }
    std::lock_guard<std::mutex> lock(dev->mu);
    mirhi_result r = drain_events(dev);
    if (r != MIRHI_OK) return r;
    for (int k = 0; k < MIRHI_KERNEL_COUNT; k++) { dev->total_ms[k] = 0; dev->launches[k] = 0; }
    dev->timeline.clear();
    if (dev->base_stop) { dev->free_events.push_back(dev->base_stop); dev->base_stop = nullptr; }
    dev->base_end_ms = 0.0;
    dev->frag_scopes = 0;
    HIP_TRY(hipMemsetAsync(dev->frag_stats, 0, 2 * sizeof(unsigned long long), dev->stream));
    HIP_TRY(hipStreamSynchronize(dev->stream));
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_get_stats(mirhi_device* dev, mirhi_device_stats* out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    drain_submits(dev);
    std::lock_guard<std::mutex> lock(dev->mu);
    *out = dev->stats;
    out->native_dispatches = dev->native ? (uint32_t)dev->native->dispatches.load(std::memory_order_relaxed) : 0u;
    out->dispatch_path = 0u;
    if (dev->native && dev->native->ok) {
        out->dispatch_path = 1u;
        for (const NativeQueue* nq : dev->native_lanes) if (nq && nq->proxy) out->dispatch_path = 2u;
    }
    out->device_lost = dev->native && dev->native->lost.load(std::memory_order_acquire) ? 1u : 0u;
    out->reserved = 0u;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_dispatch_path(mirhi_device* dev, char* out, uint32_t out_len) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out, "out");
    if (out_len == 0) return MIRHI_OK;
    std::lock_guard<std::mutex> lock(dev->mu);
    if (dev->native && dev->native->ok) {
        bool proxy = false;
        for (const NativeQueue* nq : dev->native_lanes) proxy |= nq && nq->proxy;
        snprintf(out, out_len, "native: AQL packets on the device's own ROCr queues%s%s", proxy ? " (queue intercepted by a tool: every packet keeps its barrier bit)" : "",
                 (!dev->owns_stream && !dev->native_on_external) ? "; lane 0 stays on the caller's HIP stream" : "");
    } else snprintf(out, out_len, "hip: %s", dev->native ? dev->native->why.c_str() : "native dispatcher not opened");
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_set_native_dispatch(mirhi_device* dev, uint32_t enable) {
    NULL_CHECK(dev, "device");
    mirhi_result r = sync_all_lanes(dev);          // (a lane changes the queue it submits to: nothing may be in flight across the switch)
    if (r != MIRHI_OK) return r;
    std::lock_guard<std::mutex> lock(dev->mu);
    dev->native_on_external = enable != 0;
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_device_measure_roundtrip(mirhi_device* dev, uint32_t lane, uint32_t reps, double* out_us) {
    NULL_CHECK(dev, "device"); NULL_CHECK(out_us, "out_us");
    out_us[0] = out_us[1] = 0.0;
    mirhi_result r = sync_all_lanes(dev);
    if (r != MIRHI_OK) return r;
    std::unique_lock<std::mutex> lock(dev->mu);
    NativeQueue* nq = native_lane(dev, lane);
    if (!nq) return fail(MIRHI_ERR_LOADING, "Loading error: native dispatch unavailable: %s", dev->native ? dev->native->why.c_str() : "not opened");
    lock.unlock();
    if (reps == 0) reps = 1;
    hsa_signal_t sig;
    if (hsa_signal_create(0, 0, nullptr, &sig) != HSA_STATUS_SUCCESS) return fail(MIRHI_ERR_DEVICE, "Vulkan error: hsa_signal_create failed");
    for (int what = 0; what < 2; what++) {
        double total = 0.0;
        for (uint32_t i = 0; i < reps + 8u; i++) {
            hsa_signal_store_relaxed(sig, 1);
            const auto t0 = std::chrono::steady_clock::now();
            if (what == 0) {
                const hipError_t e = launch_noop(nq, sig.handle);
                if (e != hipSuccess) { (void)hsa_signal_destroy(sig); return dev->native->lost.load() ? device_lost(dev) : hip_fail(e, "noop dispatch"); }
            } else {
                std::lock_guard<std::mutex> qlock(nq->mu);
                if (!native_reserve(nq)) { (void)hsa_signal_destroy(sig); return device_lost(dev); }
                auto* p = reinterpret_cast<hsa_barrier_and_packet_t*>(nq->q->base_address) + (nq->widx & (NATIVE_QUEUE_PACKETS - 1));
                memset(reinterpret_cast<uint8_t*>(p) + 4, 0, sizeof *p - 4);
                p->completion_signal = sig;
                native_publish(nq, p, (HSA_PACKET_TYPE_BARRIER_AND << HSA_PACKET_HEADER_TYPE) | (1 << HSA_PACKET_HEADER_BARRIER) |
                                      (HSA_FENCE_SCOPE_AGENT << HSA_PACKET_HEADER_SCACQUIRE_FENCE_SCOPE) | (HSA_FENCE_SCOPE_SYSTEM << HSA_PACKET_HEADER_SCRELEASE_FENCE_SCOPE), 0);
            }
            if (native_signal_wait(sig, UINT64_MAX, dev->native, nq, "round-trip measurement") != 0) { (void)hsa_signal_destroy(sig); return device_lost(dev); }
            if (i >= 8u) total += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        }
        out_us[what] = total / reps;
    }
    (void)hsa_signal_destroy(sig);
    return MIRHI_OK;
}

// ------------------------------------------------------------------------------------------------
// multi-GPU: exchange of the finished bands over RCCL
// ------------------------------------------------------------------------------------------------
namespace {
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    std::string error;
};
std::mutex g_rccl_mu;
Rccl g_rccl;

// The library a process already holds (PyTorch ships its own librccl.so.1) is found by its soname; otherwise the ROCm install.
mirhi_result rccl_load(Rccl** out) {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    Rccl& R = g_rccl;
    if (!R.handle) {
        const char* env = getenv("MIRHI_RCCL_LIBRARY");
        const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            if (!n || !*n) continue;
            R.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (R.handle) break;
            R.error = dlerror();
        }
        if (!R.handle) return fail(MIRHI_ERR_LOADING, "Loading error: librccl not found (%s); the tile-row split needs RCCL", R.error.c_str());
        bool ok = true;
#define MIRHI_RCCL_SYM(field, name) do { R.field = reinterpret_cast<decltype(R.field)>(dlsym(R.handle, name)); if (!R.field) { ok = false; R.error = name; } } while (0)
        MIRHI_RCCL_SYM(GetUniqueId, "ncclGetUniqueId"); MIRHI_RCCL_SYM(CommInitRank, "ncclCommInitRank"); MIRHI_RCCL_SYM(CommDestroy, "ncclCommDestroy");
        MIRHI_RCCL_SYM(CommCount, "ncclCommCount"); MIRHI_RCCL_SYM(GroupStart, "ncclGroupStart"); MIRHI_RCCL_SYM(GroupEnd, "ncclGroupEnd");
        MIRHI_RCCL_SYM(Send, "ncclSend"); MIRHI_RCCL_SYM(Recv, "ncclRecv"); MIRHI_RCCL_SYM(Broadcast, "ncclBroadcast");
        MIRHI_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef MIRHI_RCCL_SYM
        if (!ok) { dlclose(R.handle); R.handle = nullptr; return fail(MIRHI_ERR_LOADING, "Loading error: librccl lacks %s", R.error.c_str()); }
    }
    *out = &R;
    return MIRHI_OK;
}
}  // namespace

struct mirhi_comm {
    mirhi_device* dev;
    Rccl* rccl;
    ncclComm_t comm;
    uint32_t rank, world, counted;
    // Every exchange runs on ONE stream of the communicator's own, whatever queue lane rendered the frame: RCCL sees a single,
    // totally ordered stream, and frames in flight on other lanes keep rendering while a band exchange is under way.
    hipStream_t stream;
    hipEvent_t ready, done;       // lane -> exchange stream, exchange stream -> lane
    // Interleaved tile rows: a rank's share of the frame is one 32-row piece per tile row it owns, a tile row of the frame apart.  Sending the pieces one by
    // one would put (world - 1) x 2 x ~9 point-to-point operations into the group for a 4K frame on 8 ranks; instead the share is packed into slot `rank` of
    // this buffer (one strided device-to-device copy), ONE message per peer goes out of it and ONE comes into every other slot -- the op count of the
    // band layout -- and the received slots are scattered into the frame (one strided copy per peer).  [world][slot_bytes], grown on demand.
    uint8_t* pack = nullptr; size_t pack_bytes = 0;
    // A frame that left the library as AQL packets (native dispatch) is followed on its queue by one single-lane kernel that stores the exchange's sequence
    // number into `seq_word` (signal memory), and the exchange stream waits for that value (hipStreamWaitValue64): the stream is ordered behind the
    // frame's raster kernel without the host waiting for anything.
    uint64_t* seq_word = nullptr; uint64_t seq = 0;
};
#define RCCL_TRY(R, expr)                                                                                     \
    do {                                                                                                      \
        ncclResult_t r__ = (expr);                                                                            \
        if (r__ != ncclSuccess) return fail(MIRHI_ERR_DEVICE, "Vulkan error: RCCL: %s (%s)", (R)->GetErrorString(r__), #expr); \
    } while (0)

extern "C" mirhi_result mirhi_comm_unique_id(uint8_t* id) {
    NULL_CHECK(id, "id");
    static_assert(MIRHI_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    Rccl* R = nullptr;
    mirhi_result r = rccl_load(&R);
    if (r != MIRHI_OK) return r;
    ncclUniqueId u;
    RCCL_TRY(R, R->GetUniqueId(&u));
    memcpy(id, u.internal, MIRHI_COMM_ID_BYTES);
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_comm_create(mirhi_device* dev, const uint8_t* id, uint32_t rank, uint32_t world, mirhi_comm** out) {
    NULL_CHECK(dev, "device"); NULL_CHECK(id, "id"); NULL_CHECK(out, "out");
    *out = nullptr;
    if (world == 0 || rank >= world) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: communicator rank %u of %u", rank, world);
    Rccl* R = nullptr;
    mirhi_result r = rccl_load(&R);
    if (r != MIRHI_OK) return r;
    HIP_TRY(hipSetDevice(dev->ordinal));
    ncclUniqueId u;
    memcpy(u.internal, id, MIRHI_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    RCCL_TRY(R, R->CommInitRank(&comm, (int)world, u, (int)rank));
    int counted = 0;
    RCCL_TRY(R, R->CommCount(comm, &counted));
    mirhi_comm* c = new (std::nothrow) mirhi_comm{dev, R, comm, rank, world, (uint32_t)counted, nullptr, nullptr, nullptr};
    if (!c) { (void)R->CommDestroy(comm); return fail(MIRHI_ERR_ALLOCATOR, "Allocator error: host allocation failed"); }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&c->ready, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError(); (void)R->CommDestroy(comm); delete c;
        return fail(MIRHI_ERR_DEVICE, "Vulkan error: stream / event creation for the band exchange failed");
    }
    // signal memory for ordering the exchange stream behind natively dispatched frames (without it the host waits for the frame instead)
    { void* w = nullptr; if (hipExtMallocWithFlags(&w, 8, hipMallocSignalMemory) == hipSuccess) { c->seq_word = (uint64_t*)w; *c->seq_word = 0; } else (void)hipGetLastError(); }
    { std::lock_guard<std::mutex> lk(dev->mu); dev->aux_streams.push_back(c->stream); }
    dev->split_rank = rank; dev->split_world = world;
    dev->children++;
    *out = c;
    return MIRHI_OK;
}
extern "C" uint32_t mirhi_comm_world(const mirhi_comm* comm) { return comm ? comm->counted : 0; }
extern "C" uint32_t mirhi_comm_rank(const mirhi_comm* comm) { return comm ? comm->rank : 0; }

extern "C" mirhi_result mirhi_comm_all_gather_bands(mirhi_comm* comm, mirhi_image* frame, mirhi_cmd* after, mirhi_gather_algo algo) {
    NULL_CHECK(comm, "comm"); NULL_CHECK(frame, "frame");
    REFUSE_MULTISAMPLED(frame, "gathered");
    mirhi_device* dev = comm->dev;
    if (frame->dev != dev || (after && after->dev != dev)) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: frame / command buffer belongs to another device");
    if (algo != MIRHI_GATHER_DIRECT && algo != MIRHI_GATHER_BROADCAST) return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: unknown gather algorithm %d", (int)algo);
    if (dev->split_world != comm->world || dev->split_rank != comm->rank)
        return fail(MIRHI_ERR_INVALID_HANDLE, "Invalid handle: the device's tile split (%u of %u) is not the communicator's (%u of %u)", dev->split_rank, dev->split_world, comm->rank, comm->world);
    drain_submits(dev);
    HIP_TRY(hipSetDevice(dev->ordinal));
    hipStream_t lane = after && after->last_stream ? after->last_stream : dev->lanes[after && after->lane < dev->lanes.size() ? after->lane : 0];
    NativeQueue* const native_after = (after && after->last_native && comm->seq_word) ? after->last_native : nullptr;
    if (after && after->last_native && !native_after && !drain_native(dev, after->last_native)) return device_lost(dev);     // (no signal memory: the host waits for the frame)
    hipStream_t stream = comm->stream;
    dev->foreign_writes++;                                   // (peers write the other ranks' rows into this frame)
    const uint32_t tiles_y = (frame->height + TILE - 1) / TILE;
    const size_t row_bytes = (size_t)frame->width * format_bpp(frame->format);
    const size_t tile_row_bytes = (size_t)TILE * row_bytes;
    Rccl* R = comm->rccl;
    // rank r's share: tile rows first + k * step, k < count; the frame's last tile row may be short
    struct Share { uint32_t first, step, count; size_t bytes; };
    auto share = [&](uint32_t r) {
        Share sh{0, 1, 0, 0};
        split_rows(dev->split_layout, r, comm->world, tiles_y, &sh.first, &sh.step, &sh.count);
        for (uint32_t k = 0; k < sh.count; k++) {
            const size_t p0 = (size_t)(sh.first + k * sh.step) * TILE, p1 = std::min<size_t>(p0 + TILE, frame->height);
            sh.bytes += (p1 > p0 ? p1 - p0 : 0) * row_bytes;
        }
        return sh;
    };
    const Share mine = share(comm->rank);
    if (comm->world == 1) return MIRHI_OK;
    const bool packed = dev->split_layout == MIRHI_SPLIT_INTERLEAVED;
    const size_t slot_bytes = ((tiles_y + comm->world - 1) / comm->world) * tile_row_bytes;
    if (packed && comm->pack_bytes < slot_bytes * comm->world) {
        HIP_TRY(hipStreamSynchronize(stream));
        if (comm->pack) { (void)hipFree(comm->pack); comm->pack = nullptr; comm->pack_bytes = 0; }
        HIP_TRY(hipMalloc((void**)&comm->pack, slot_bytes * comm->world));
        comm->pack_bytes = slot_bytes * comm->world;
    }
    // strided copy between a rank's rows in the frame and its slot of the pack buffer (to_slot: gather, else scatter); the last tile row of the frame may be short
    auto strided = [&](const Share& sh, uint8_t* slot, bool to_slot) -> hipError_t {
        if (!sh.count) return hipSuccess;
        uint8_t* rows = frame->ptr + (size_t)sh.first * tile_row_bytes;
        const size_t pitch = (size_t)sh.step * tile_row_bytes;
        const size_t last_p0 = (size_t)(sh.first + (sh.count - 1) * sh.step) * TILE;
        const size_t last_bytes = (std::min<size_t>(last_p0 + TILE, frame->height) - last_p0) * row_bytes;
        const uint32_t full = last_bytes == tile_row_bytes ? sh.count : sh.count - 1;
        hipError_t e = hipSuccess;
        if (full) e = to_slot ? hipMemcpy2DAsync(slot, tile_row_bytes, rows, pitch, tile_row_bytes, full, hipMemcpyDeviceToDevice, stream)
                              : hipMemcpy2DAsync(rows, pitch, slot, tile_row_bytes, tile_row_bytes, full, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess && full < sh.count && last_bytes)
            e = to_slot ? hipMemcpyAsync(slot + (size_t)full * tile_row_bytes, rows + (size_t)full * pitch, last_bytes, hipMemcpyDeviceToDevice, stream)
                        : hipMemcpyAsync(rows + (size_t)full * pitch, slot + (size_t)full * tile_row_bytes, last_bytes, hipMemcpyDeviceToDevice, stream);
        return e;
    };
    // the exchange starts behind the frame's raster kernel ...
    if (native_after) {
        const uint64_t want = ++comm->seq;
        { const hipError_t ne = launch_seq_store(native_after, comm->seq_word, want); if (ne != hipSuccess) return dev->native->lost.load() ? device_lost(dev) : hip_fail(ne, "sequence store behind the frame"); }
        HIP_TRY(hipStreamWaitValue64(stream, comm->seq_word, want, hipStreamWaitValueGte, ~0ull));
    } else {
        HIP_TRY(hipEventRecord(comm->ready, lane));
        HIP_TRY(hipStreamWaitEvent(stream, comm->ready, 0));
    }
    if (packed) HIP_TRY(strided(mine, comm->pack + comm->rank * slot_bytes, true));
    RCCL_TRY(R, R->GroupStart());
    // Inside the group nothing returns early: a failing call must not leave the thread's RCCL group open (every later RCCL call of
    // this thread, torch.distributed's included, would queue into a group that never ends).  The first error is kept, the group is
    // closed, and only a successful exchange makes the lane wait for it.
    ncclResult_t first = ncclSuccess; const char* what = "";
    auto note = [&](ncclResult_t rc, const char* call) { if (rc != ncclSuccess && first == ncclSuccess) { first = rc; what = call; } };
    uint8_t* const my_ptr = packed ? comm->pack + comm->rank * slot_bytes : frame->ptr + (size_t)mine.first * tile_row_bytes;
    for (uint32_t r = 0; r < comm->world && first == ncclSuccess; r++) {
        const Share sh = share(r);
        uint8_t* const ptr = packed ? comm->pack + r * slot_bytes : frame->ptr + (size_t)sh.first * tile_row_bytes;
        if (algo == MIRHI_GATHER_BROADCAST) {
            if (sh.bytes) note(R->Broadcast(ptr, ptr, sh.bytes, ncclUint8, (int)r, comm->comm, stream), "ncclBroadcast");
            continue;
        }
        if (r == comm->rank) continue;
        if (mine.bytes) note(R->Send(my_ptr, mine.bytes, ncclUint8, (int)r, comm->comm, stream), "ncclSend");
        if (sh.bytes && first == ncclSuccess) note(R->Recv(ptr, sh.bytes, ncclUint8, (int)r, comm->comm, stream), "ncclRecv");
    }
    note(R->GroupEnd(), "ncclGroupEnd");
    if (first != ncclSuccess) return fail(MIRHI_ERR_DEVICE, "Vulkan error: RCCL: %s (%s)", R->GetErrorString(first), what);
    if (packed) for (uint32_t r = 0; r < comm->world; r++) if (r != comm->rank) HIP_TRY(strided(share(r), comm->pack + r * slot_bytes, false));
    // ... and whatever touches the frame next waits for the exchange: a HIP lane through an event, an AQL queue through the frame's attachment record
    // (order_attachments: the exchange stream is this image's last user)
    HIP_TRY(hipEventRecord(comm->done, stream));
    if (!native_after) HIP_TRY(hipStreamWaitEvent(lane, comm->done, 0));
    { std::lock_guard<std::mutex> lk(dev->mu); frame->last_stream = stream; frame->last_native = nullptr; frame->last_cmd = nullptr; frame->last_seq = 0; }
    return MIRHI_OK;
}
extern "C" mirhi_result mirhi_comm_destroy(mirhi_comm* comm) {
    NULL_CHECK(comm, "comm");
    (void)hipSetDevice(comm->dev->ordinal);
    (void)sync_all_lanes(comm->dev);
    (void)hipStreamSynchronize(comm->stream);
    (void)comm->rccl->CommDestroy(comm->comm);
    (void)hipEventDestroy(comm->ready); (void)hipEventDestroy(comm->done);
    { std::lock_guard<std::mutex> lk(comm->dev->mu); auto& v = comm->dev->aux_streams; v.erase(std::remove(v.begin(), v.end(), comm->stream), v.end());
      for (mirhi_image* img : comm->dev->images) if (img->last_stream == comm->stream) img->last_stream = nullptr; }
    (void)hipStreamDestroy(comm->stream);
    if (comm->pack) (void)hipFree(comm->pack);
    if (comm->seq_word) (void)hipFree(comm->seq_word);
    comm->dev->children--;
    delete comm;
    return MIRHI_OK;
}
