// hk_api.hip -- C-ABI host layer of libhomonim_hk.so (declared in include/homonim_hk.h).
//
// Owns: one HIP device per context, a pool of streams each with a device staging slab, argument validation
// (mirrors homonim/utils.py:104-133 and homonim/kernel_model.py:430-431,459-460 error behaviour as status codes),
// and the dispatch to the gfx950 kernels in hk_fit_kernel.h (through hk_kernels.hip) / hk_norm.hip.  No global mutable state besides the
// thread-local error string; any number of host threads may use one context (homonim/fuse.py:396-401).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cctype>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <optional>
#include <type_traits>
#include <vector>

#include "../../include/homonim_hk.h"
#include "../../include/homonim_hk_devtools.h"
#include "hk_kernels.h"

#include <dlfcn.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>  // types only: the loaded HSA runtime is looked up at run time (gpu_fault_report)
#include <rccl/rccl.h>  // types and prototypes only: librccl is opened at run time (hk_comm_*), not linked

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// HIP keeps a per-thread "last error" until somebody reads it, and the launch wrappers of the kernel files report their
// launches through hipGetLastError(): a failure this layer hands back to a caller who carries on (e.g. hk_host_register of
// memory that is page-locked already) would otherwise surface again as the status of that thread's NEXT launch.  So a
// failing call clears the state it leaves behind, and every entry point that selects the device starts from a clean slate.
#define HK_HIP(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) {                                                                            \
            (void)hipGetLastError();                                                                       \
            return fail(HK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
        }                                                                                                  \
    } while (0)
#define HK_ENTER(ctx)                         \
    do {                                      \
        HK_HIP(hipSetDevice((ctx)->device));  \
        (void)hipGetLastError();              \
    } while (0)

// Every device allocation of the library goes through dev_malloc / dev_free.  HK_GUARD_ALLOC=lo|hi (a debugging switch: GPU
// AddressSanitizer is not available everywhere) places each allocation in its own mapping of the virtual-memory API with
// UNMAPPED address ranges on both sides, its first byte at the start of the mapping (lo: reads or writes below the buffer
// fault) or its last 256-byte unit at the end (hi: those above it do), so an out-of-range access of a kernel ends the
// process at that launch instead of reading whatever happens to be mapped next to the buffer.
struct GuardedRange {
    void* user;
    void* va;
    size_t va_bytes;
    void* mapped;
    size_t mapped_bytes;
    hipMemGenericAllocationHandle_t handle;
};
int guard_mode() {  // 0 off, 1 lo, 2 hi
    static const int mode = [] {
        const char* e = getenv("HK_GUARD_ALLOC");
        if (!e || !*e || !strcmp(e, "0")) return 0;
        if (!strcmp(e, "poison")) return 3;  // plain hipMalloc, contents set to 0xAB: nothing may rely on fresh memory being zero
        return !strcmp(e, "hi") ? 2 : 1;
    }();
    return mode;
}
std::mutex g_guard_mu;
std::vector<GuardedRange> g_guarded;

// What the library has allocated on the device (a handful of slabs, workspaces and the callers' hk_dev_alloc buffers): a GPU
// memory fault is reported with its place relative to them (gpu_fault_report).
struct DevRange {
    uintptr_t base;
    size_t bytes;
};
std::mutex g_ranges_mu;
std::vector<DevRange> g_ranges;
void note_alloc(void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_ranges_mu);
    g_ranges.push_back({reinterpret_cast<uintptr_t>(p), bytes});
}
void note_free(void* p) {
    std::lock_guard<std::mutex> lk(g_ranges_mu);
    for (size_t i = 0; i < g_ranges.size(); ++i)
        if (g_ranges[i].base == reinterpret_cast<uintptr_t>(p)) {
            g_ranges[i] = g_ranges.back();
            g_ranges.pop_back();
            return;
        }
}

// A GPU memory fault (or hardware exception) ends the process with an abort() of the HSA runtime's event thread; the runtime names
// the address, not what it belongs to.  The library registers a system-event callback of its own that says where the address
// lies relative to the library's allocations, and then lets the runtime carry on as before (it does not claim to have handled
// the event).
hsa_status_t gpu_fault_report(const hsa_amd_event_t* ev, void*) {
    if (!ev) return HSA_STATUS_ERROR;
    if (ev->event_type == HSA_AMD_GPU_MEMORY_FAULT_EVENT || ev->event_type == HSA_AMD_GPU_MEMORY_ERROR_EVENT) {
        const bool fault = ev->event_type == HSA_AMD_GPU_MEMORY_FAULT_EVENT;
        const uint64_t addr = fault ? ev->memory_fault.virtual_address : ev->memory_error.virtual_address;
        const uint32_t mask = fault ? ev->memory_fault.fault_reason_mask : ev->memory_error.error_reason_mask;
        char where[200] = "not near any allocation of libhomonim_hk";
        {
            std::lock_guard<std::mutex> lk(g_ranges_mu);
            uint64_t best = ~0ull;
            for (const DevRange& r : g_ranges) {
                if (addr >= r.base && addr < r.base + r.bytes) {
                    snprintf(where, sizeof where, "INSIDE a library allocation of %zu bytes (offset %llu): freed or remapped under a kernel?",
                             r.bytes, (unsigned long long)(addr - r.base));
                    best = 0;
                    break;
                }
                const uint64_t d = addr < r.base ? r.base - addr : addr - (r.base + r.bytes) + 1;
                if (d < best && d < (64ull << 20)) {
                    best = d;
                    if (addr < r.base)
                        snprintf(where, sizeof where, "%llu bytes BELOW a library allocation of %zu bytes", (unsigned long long)d, r.bytes);
                    else
                        snprintf(where, sizeof where, "%llu bytes past the END of a library allocation of %zu bytes",
                                 (unsigned long long)(d - 1), r.bytes);
                }
            }
        }
        fprintf(stderr, "[libhomonim_hk] GPU memory %s at 0x%llx, reason mask 0x%x%s%s%s%s: %s\n", fault ? "access fault" : "error",
                (unsigned long long)addr, mask, (fault && (mask & HSA_AMD_MEMORY_FAULT_PAGE_NOT_PRESENT)) ? " page-not-present" : "",
                (fault && (mask & HSA_AMD_MEMORY_FAULT_READ_ONLY)) ? " read-only" : "",
                (fault && (mask & (HSA_AMD_MEMORY_FAULT_DRAMECC | HSA_AMD_MEMORY_FAULT_SRAMECC))) ? " ECC" : "",
                (fault && (mask & HSA_AMD_MEMORY_FAULT_HANG)) ? " hang/reset" : "", where);
        fflush(stderr);
    } else if (ev->event_type == HSA_AMD_GPU_HW_EXCEPTION_EVENT) {
        fprintf(stderr, "[libhomonim_hk] GPU hardware exception: reset type 0x%x, cause 0x%x%s%s\n", (unsigned)ev->hw_exception.reset_type,
                (unsigned)ev->hw_exception.reset_cause,
                (ev->hw_exception.reset_cause & HSA_AMD_HW_EXCEPTION_CAUSE_GPU_HANG) ? " GPU hang" : "",
                (ev->hw_exception.reset_cause & HSA_AMD_HW_EXCEPTION_CAUSE_ECC) ? " ECC" : "");
        fflush(stderr);
    }
    return HSA_STATUS_ERROR;  // not handled here: the runtime's own handling (ending the process) follows
}
void register_gpu_fault_report() {
    static std::once_flag once;
    std::call_once(once, [] {
        const char* on = getenv("HK_FAULT_REPORT");  // opt-in: a process-wide callback is not a library call's business
        if (!on || strcmp(on, "1")) return;
        void* hsa = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_NOLOAD);  // the instance HIP runs on, or nothing
        if (!hsa) return;
        using reg_t = hsa_status_t (*)(hsa_amd_system_event_callback_t, void*);
        reg_t reg = reinterpret_cast<reg_t>(dlsym(hsa, "hsa_amd_register_system_event_handler"));
        if (reg) (void)reg(gpu_fault_report, nullptr);
    });
}

// does a buffer of `have` bytes serve a request for `need`?  (guarded: only an exact fit, so that the request's end is the mapping's)
bool fits(size_t have, size_t need) { return guard_mode() ? have == need : have >= need; }

hipError_t dev_malloc(void** out, size_t bytes) {
    if (!guard_mode()) {
        const hipError_t pe = hipMalloc(out, bytes);
        if (pe == hipSuccess) note_alloc(*out, bytes);
        return pe;
    }
    if (guard_mode() == 3) {
        hipError_t pe = hipMalloc(out, bytes);
        if (pe == hipSuccess) note_alloc(*out, bytes);
        if (pe == hipSuccess) pe = hipMemset(*out, 0xAB, bytes);
        if (pe == hipSuccess) pe = hipDeviceSynchronize();
        return pe;
    }
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    if ((e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum)) != hipSuccess) return e;
    const size_t unit = (std::max<size_t>(bytes, 1) + 255) / 256 * 256;
    GuardedRange g = {};
    g.mapped_bytes = (unit + gran - 1) / gran * gran;
    g.va_bytes = g.mapped_bytes + 2 * gran;
    if ((e = hipMemAddressReserve(&g.va, g.va_bytes, gran, nullptr, 0)) != hipSuccess) return e;
    g.mapped = static_cast<char*>(g.va) + gran;
    if ((e = hipMemCreate(&g.handle, g.mapped_bytes, &prop, 0)) != hipSuccess) {
        (void)hipMemAddressFree(g.va, g.va_bytes);
        return e;
    }
    hipMemAccessDesc access = {};
    access.location = prop.location;
    access.flags = hipMemAccessFlagsProtReadWrite;
    if ((e = hipMemMap(g.mapped, g.mapped_bytes, 0, g.handle, 0)) != hipSuccess ||
        (e = hipMemSetAccess(g.mapped, g.mapped_bytes, &access, 1)) != hipSuccess) {
        (void)hipMemUnmap(g.mapped, g.mapped_bytes);
        (void)hipMemRelease(g.handle);
        (void)hipMemAddressFree(g.va, g.va_bytes);
        return e;
    }
    g.user = guard_mode() == 2 ? static_cast<char*>(g.mapped) + (g.mapped_bytes - unit) : g.mapped;
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        g_guarded.push_back(g);
    }
    *out = g.user;
    note_alloc(g.user, unit);
    // poison + synchronise: nothing may rely on fresh memory being zero, and a kernel queued right behind hipMemSetAccess
    // on a non-blocking stream was seen to read the new range before its mapping had settled (wrong values, no fault)
    e = hipMemset(g.mapped, 0xAB, g.mapped_bytes);
    return e != hipSuccess ? e : hipDeviceSynchronize();
}

hipError_t dev_free(void* p) {
    if (p) note_free(p);
    if (!guard_mode() || guard_mode() == 3 || !p) return hipFree(p);
    GuardedRange g = {};
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        for (size_t i = 0; i < g_guarded.size(); ++i)
            if (g_guarded[i].user == p) {
                g = g_guarded[i];
                g_guarded.erase(g_guarded.begin() + i);
                break;
            }
    }
    if (!g.user) return hipFree(p);  // not one of ours (allocated before the switch was read: cannot happen; or foreign)
    hipError_t e = hipDeviceSynchronize();  // hipFree's implicit synchronisation
    if (e != hipSuccess) return e;
    // the address range stays reserved (and unmapped: a use after free faults as well); the physical memory goes back
    if ((e = hipMemUnmap(g.mapped, g.mapped_bytes)) != hipSuccess) return e;
    return hipMemRelease(g.handle);
}

struct Slot {
    hipStream_t stream = nullptr;
    void* dev = nullptr;      // staging slab of the host-pointer calls (owned by whoever holds the lease)
    size_t dev_bytes = 0;
    void* norm_ws = nullptr;  // workspace of hk_block_norm_dev on this stream (never shared with `dev`)
    size_t norm_ws_bytes = 0;
    void* aux = nullptr;      // on-demand planes + tables of the in-painting branch
    size_t aux_bytes = 0;
    // exchange buffer of hk_block_norm_split_comm_dev on THIS stream: sequences queued on different streams run concurrently on
    // the device (comm_mu only orders their queuing), so they must not share one
    double* comm_xchg = nullptr;
    size_t comm_xchg_bytes = 0;
    // Pinned words of the slot (PIN_BYTES of hipHostMalloc'd memory): small results and arguments travel through them,
    // never through the caller's pageable memory.  fail_host = the first word (the r2-mask failure counter).
    unsigned long long* fail_host = nullptr;
    static constexpr size_t PIN_NORM = 64, PIN_SUMS = 128, PIN_NORM_IN = 192, PIN_WORD = 256, PIN_STATS = 512, PIN_COUNTS = 1024, PIN_BYTES = 16384;
    template <class T> T* pin(size_t off) const { return reinterpret_cast<T*>(reinterpret_cast<char*>(fail_host) + off); }
    // Pinned staging ring of the host-pointer calls (stage_h2d / stage_d2h below): STAGE_N chunks of stage_chunk bytes.
    // A chunk is re-used once the copy that last used it has completed (stage_ev); a device-to-host chunk additionally
    // carries the unpacking into the caller's array that follows its copy.
    static constexpr int STAGE_N = 4;
    struct StageOut {
        char* h_dst = nullptr;
        size_t h_pitch = 0, row_bytes = 0, c_pitch = 0;
        size_t rows = 0;
    };
    char* stage = nullptr;
    size_t stage_chunk = 0;
    hipEvent_t stage_ev[STAGE_N] = {nullptr, nullptr, nullptr, nullptr};
    int stage_state[STAGE_N] = {0, 0, 0, 0};  // 0 free, 1 host-to-device copy queued, 2 device-to-host copy queued (unpack follows)
    StageOut stage_out[STAGE_N];
    int stage_next = 0;
    // job / plane tables of the batched device entry points: a small ring of (pinned host, device) buffer pairs; entry i is
    // re-used once the upload recorded in tbl_ev[i] has been made (the device side is ordered by the stream itself)
    static constexpr int TBL_RING = 4;
    void* tbl_host[TBL_RING] = {nullptr, nullptr, nullptr, nullptr};
    void* tbl_dev[TBL_RING] = {nullptr, nullptr, nullptr, nullptr};
    size_t tbl_bytes[TBL_RING] = {0, 0, 0, 0};
    hipEvent_t tbl_ev[TBL_RING] = {nullptr, nullptr, nullptr, nullptr};
    int tbl_next = 0;
    // gain-offset with the r2 mask: the wave-rows the certificate build leaves to the list launch (FitArgs::open_rows), one bit each
    unsigned* open_rows = nullptr;
    size_t open_rows_bytes = 0;
    bool direct_pending = false;  // copies queued straight from / to page-locked CALLER arrays since the last stream synchronisation
    bool busy = false;         // leased by a host-pointer call (SlotLease)
    int dev_inflight = 0;      // device-job entry points currently queuing on this stream (DevEnter): a lease waits for them
    bool dev_touched = false;  // device-resident jobs were queued on this stream since the last lease drained it
};

constexpr int64_t ROW_ALIGN = 64;  // device rows padded to 64 elements (256 B)
int64_t row_align(int64_t w) { return (w + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN; }

// The launch switches of the environment (README "Environment switches"), read once per context by hk_ctx_create.
struct LaunchPolicy {
    // runs of this many consecutive units (neighbouring strips) per XCD, 0 = plain round-robin (hk_fit_kernel.h); 16 measured
    // best across models on MI355X (gain 5x5: -12 %, gain-offset without the r2 mask: -4 %, VALU-bound variants: -1 %)
    int xcd_remap = 16;
    int force_general = 0;              // HK_FORCE_GENERAL: never take the dense specialisation (testing)
    std::optional<int> use_ring;        // HK_USE_RING: a ring mode forced where the shape has a build of it (testing)
    int wave_slots = 256 * 12;          // HK_WAVE_SLOTS: resident waves of the device (3 per SIMD), seg_policy()
    std::optional<int> seg_big, seg_tail;  // HK_SEG_BIG / HK_SEG_TAIL: the two segment heights of seg_policy()
};

}  // namespace

struct hk_ctx {
    int device = 0;
    std::vector<Slot> slots;
    std::mutex mu;
    std::condition_variable cv;
    LaunchPolicy launch;
    // the last HOST-POINTER gain-offset call with a threshold found pixels failing the r2 mask: real imagery usually does, block
    // after block, so the next call lets its first pass leave what the in-painting reads (offsets + source flags, 5 bytes per
    // pixel of stores) instead of running it again when the count comes back non-zero.  Either choice gives the same results.
    std::atomic<int> expect_r2_failures{0};
    // RCCL communicator of the one data-path collective (hk_comm_init; the split-block statistics)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 0;
    std::mutex comm_mu;          // collectives of one communicator are queued in one order on every rank
    // hk_memcpy_h2d / hk_memcpy_d2h / hk_selftest: a stream + pinned staging ring of their own, one caller at a time
    Slot xfer;
    std::mutex xfer_mu;
};

struct hk_event {
    hipEvent_t ev;
};

namespace {

void stage_abandon(Slot& s);  // (host staging, below)

struct SlotLease {
    hk_ctx* ctx;
    int idx;
    // Host-pointer calls and device-resident jobs share the pooled streams and their scratch (norm_ws, aux).  The rule "do
    // not mix them on one context concurrently" is enforced here instead of being left to the caller: a lease prefers a
    // stream no device job has touched; if it has to take one that was, it drains that stream first (the jobs queued on it
    // are complete before the slot's scratch is re-used), and a device-job call waits while its stream is leased
    // (dev_slot_enter below).
    SlotLease(hk_ctx* c) : ctx(c), idx(-1) {
        bool drain = false;
        {
            std::unique_lock<std::mutex> lk(ctx->mu);
            ctx->cv.wait(lk, [&] {
                int any = -1;
                for (size_t i = 0; i < ctx->slots.size(); ++i) {
                    if (ctx->slots[i].busy || ctx->slots[i].dev_inflight > 0) continue;
                    if (!ctx->slots[i].dev_touched) {
                        idx = (int)i;
                        return true;
                    }
                    if (any < 0) any = (int)i;
                }
                idx = any;
                return any >= 0;
            });
            ctx->slots[idx].busy = true;
            drain = ctx->slots[idx].dev_touched;
            ctx->slots[idx].dev_touched = false;
        }
        if (drain) (void)hipStreamSynchronize(ctx->slots[idx].stream);
    }
    ~SlotLease() {
        // a call that ends through stage_finish() leaves no chunk queued; one that returned an error earlier does -- see stage_abandon
        stage_abandon(ctx->slots[idx]);
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            ctx->slots[idx].busy = false;
        }
        ctx->cv.notify_all();
    }
    Slot& slot() { return ctx->slots[idx]; }
};

// A device-resident job is about to be queued on pooled stream `stream`: wait for a host-pointer call that holds it, and keep
// the slot from being leased until the entry point has finished queuing (it uses the slot's scratch -- norm_ws, aux, the table
// ring -- after this check; a lease taken in between would drain an still-empty stream and use the same scratch).
struct DevEnter {
    hk_ctx* ctx;
    int stream;
    DevEnter(hk_ctx* c, int st) : ctx(c), stream(st) {
        std::unique_lock<std::mutex> lk(ctx->mu);
        ctx->cv.wait(lk, [&] { return !ctx->slots[stream].busy; });
        ctx->slots[stream].dev_touched = true;
        ++ctx->slots[stream].dev_inflight;
    }
    ~DevEnter() {
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            --ctx->slots[stream].dev_inflight;
        }
        ctx->cv.notify_all();
    }
    DevEnter(const DevEnter&) = delete;
    DevEnter& operator=(const DevEnter&) = delete;
};

// RCCL, opened on first use: the library itself stays loadable (and its CPU-side tests runnable) where librccl is absent
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
RcclApi& rccl() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.lib) break;
        }
        if (!api.lib) return;
        api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.lib, "ncclGetUniqueId"));
        api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.lib, "ncclCommInitRank"));
        api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
        api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.lib, "ncclAllReduce"));
        api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce && api.GetErrorString;
    });
    return api;
}
#define HK_RCCL(expr)                                                                                         \
    do {                                                                                                      \
        ncclResult_t _r = (expr);                                                                             \
        if (_r != ncclSuccess)                                                                                \
            return fail(HK_ERR_HIP, "%s failed: %s (%s:%d)", #expr, rccl().GetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

// A grow-only device buffer of a slot (`buf`, `have` bytes): a request that fits() it keeps it; a larger one drains the slot's
// stream (work queued there may still read the buffer), frees it and allocates `need` bytes, plus `slack` unless guarded (the
// buffer then ends where its last user's does).  The caller holds whatever lock guards the slot's scratch.
template <class T>
int grow_slot_buf(Slot& s, T*& buf, size_t& have, size_t need, size_t slack = 0) {
    if (fits(have, need)) return HK_OK;
    if (buf) {
        HK_HIP(hipStreamSynchronize(s.stream));
        HK_HIP(dev_free(buf));
        buf = nullptr, have = 0;
    }
    const size_t want = guard_mode() ? need : need + slack;
    void* p = nullptr;
    if (dev_malloc(&p, want) != hipSuccess) return fail(HK_ERR_NOMEM, "hipMalloc(%zu) failed", want);
    buf = static_cast<T*>(p), have = want;
    return HK_OK;
}

// the staging slab of the host-pointer calls (an eighth to spare)
int ensure_dev(Slot& s, size_t bytes) { return grow_slot_buf(s, s.dev, s.dev_bytes, bytes, bytes / 8); }

// Bump allocation inside the staging slab: every buffer at a 256-byte aligned offset, in the order it is taken (hk_layout.h).
using hk::SlabLayout;

// How a host-pointer call opens: a leased slot whose staging slab holds `bytes` (rc says whether it does), and the buffers of
// the call's layout inside it.
struct HostCall {
    SlotLease lease;
    Slot& sl;
    const int rc;
    HostCall(hk_ctx* ctx, size_t bytes) : lease(ctx), sl(lease.slot()), rc(ensure_dev(sl, bytes)) {}
    template <class T = char> T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(sl.dev) + off); }
};

// refusals that many entry points share
int null_arg() { return fail(HK_ERR_ARG, "NULL pointer argument"); }
int check_stream(const hk_ctx* ctx, int stream) {
    return (stream < 0 || stream >= (int)ctx->slots.size()) ? fail(HK_ERR_ARG, "bad stream index") : HK_OK;
}
int check_strides(int64_t stride_a, int64_t width_a, int64_t stride_b = 0, int64_t width_b = 0) {
    return (stride_a < width_a || stride_b < width_b) ? fail(HK_ERR_ARG, "row stride smaller than width") : HK_OK;
}
int check_band_strides(int64_t a, int64_t b = 0) { return (a < 0 || b < 0) ? fail(HK_ERR_ARG, "band_stride is negative") : HK_OK; }
int check_nodata_mode(int32_t mode, int32_t last = HK_NODATA_VALUE) {  // (`last` = 3 where the coverage-fraction mode is legal)
    return (mode < 0 || mode > last) ? fail(HK_ERR_ARG, "bad nodata mode %d", mode) : HK_OK;
}
int check_nodata_modes(int32_t src_mode, int32_t ref_mode) {
    const int rc = check_nodata_mode(src_mode);
    return rc ? rc : check_nodata_mode(ref_mode);
}

// ---------------------------------------------------------------------------------------------------------------------
// Host staging.  BASELINE.json north_star: "blocks stream ... into pinned host buffers and hipMemcpyAsync to HBM".  The HIP
// runtime is only ever handed page-locked memory: the library's own ring (pack on the host -> ONE contiguous hipMemcpyAsync
// per chunk -> pitched layout on the device, and the reverse), or the caller's arrays when those are page-locked already
// (hk_host_alloc / hk_host_register: direct, fully asynchronous).  The runtime's pageable paths -- pinning caller pages on
// the fly, rect copies into unaligned few-byte rows of a numpy buffer -- are not part of the product.
constexpr size_t STAGE_CHUNK_MIN = 8u << 20;

// Page-locked host ranges this library made (hk_host_alloc, hk_host_register), process-wide: base -> bytes.  A caller array
// is handed to the runtime's copy engines directly only if ONE of these ranges holds all of it -- every row, every byte between
// the first and the last.  (Rounds 3-4 asked the runtime about the array's first and last byte: a strided view whose ends lie in
// two different registered ranges with pageable memory between them passed, and the runtime pinned the gap on the fly -- the
// path of profiles/r04_abort_caught.txt.)  Memory page-locked by other means is unknown here and goes through the staging ring.
struct PinnedRanges {
    std::mutex mu;
    std::map<uintptr_t, size_t> r;
    void add(const void* p, size_t n) {
        std::lock_guard<std::mutex> lk(mu);
        r[reinterpret_cast<uintptr_t>(p)] = n;
    }
    void remove(const void* p) {
        std::lock_guard<std::mutex> lk(mu);
        r.erase(reinterpret_cast<uintptr_t>(p));
    }
    bool covers(const void* p, size_t n) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        std::lock_guard<std::mutex> lk(mu);
        auto it = r.upper_bound(a);
        if (it == r.begin()) return false;
        --it;
        return a >= it->first && n <= it->second && a - it->first <= it->second - n;
    }
};
PinnedRanges& pinned_ranges() {
    static PinnedRanges g;
    return g;
}
// copies handed to the runtime straight from / to caller memory, and chunks that went through the staging ring (hk_debug_staging_counters)
std::atomic<unsigned long long> g_direct_copies{0}, g_staged_chunks{0};
std::atomic<int> g_fail_after_d2h{0};  // fault injection of the test-suite (hk_debug_fail_after_d2h)

// is [p, p + bytes) inside one page-locked range of this library?
bool host_is_pinned(const void* p, size_t bytes) { return bytes > 0 && pinned_ranges().covers(p, bytes); }

// HK_ASSERT_PINNED=1 (the test-suite sets it): before a caller pointer goes to hipMemcpy*Async directly, ask the runtime about
// EVERY page of every row; a page it does not know as host memory fails the call instead of being pinned on the fly.
bool assert_pinned_on() {
    static const bool on = [] { const char* e = getenv("HK_ASSERT_PINNED"); return e && atoi(e) != 0; }();
    return on;
}
int check_rows_pinned(const void* p, size_t pitch, size_t row_bytes, size_t rows) {
    const char* base = static_cast<const char*>(p);
    for (size_t r = 0; r < rows; ++r) {
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(base + r * pitch), a1 = a0 + row_bytes - 1;
        for (uintptr_t pg = a0 & ~(uintptr_t)4095; pg <= a1; pg += 4096) {
            hipPointerAttribute_t attr;
            const void* q = reinterpret_cast<const void*>(pg < a0 ? a0 : pg);
            const bool ok = hipPointerGetAttributes(&attr, q) == hipSuccess && attr.type == hipMemoryTypeHost;
            (void)hipGetLastError();
            if (!ok) return fail(HK_ERR_ARG, "HK_ASSERT_PINNED: host address %p (row %zu) is not page-locked but was about to be copied directly", q, r);
        }
    }
    return HK_OK;
}

int ensure_pin(Slot& s) {
    if (s.fail_host) return HK_OK;
    if (hipHostMalloc(reinterpret_cast<void**>(&s.fail_host), Slot::PIN_BYTES, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        s.fail_host = nullptr;
        return fail(HK_ERR_NOMEM, "hipHostMalloc(%zu) failed", (size_t)Slot::PIN_BYTES);
    }
    memset(s.fail_host, 0, Slot::PIN_BYTES);
    return HK_OK;
}

// the copy (and unpacking) that last used chunk `i` is complete
int stage_settle(Slot& s, int i) {
    if (s.stage_state[i] == 0) return HK_OK;
    HK_HIP(hipEventSynchronize(s.stage_ev[i]));
    if (s.stage_state[i] == 2) {
        const Slot::StageOut& o = s.stage_out[i];
        const char* c = s.stage + (size_t)i * s.stage_chunk;
        if (o.h_pitch == o.row_bytes && o.c_pitch == o.row_bytes) memcpy(o.h_dst, c, o.rows * o.row_bytes);
        else
            for (size_t r = 0; r < o.rows; ++r) memcpy(o.h_dst + r * o.h_pitch, c + r * o.c_pitch, o.row_bytes);
    }
    s.stage_state[i] = 0;
    return HK_OK;
}

// every queued staging copy of the slot has completed and has been unpacked (the caller's output arrays are final)
int stage_drain(Slot& s) {
    if (!s.stage) return HK_OK;
    for (int k = 0; k < Slot::STAGE_N; ++k) {
        const int rc = stage_settle(s, (s.stage_next + k) % Slot::STAGE_N);  // oldest first
        if (rc) return rc;
    }
    return HK_OK;
}

// A byte cap of a chunked path: the environment variable `name_kb`, in KiB, sets it for the tests of that path; unset, empty
// or not positive: `dflt`
size_t cap_from_env(const char* name_kb, size_t dflt) {
    const char* e = getenv(name_kb);
    return (e && atol(e) > 0) ? (size_t)atol(e) << 10 : dflt;
}

int ensure_stage(Slot& s, size_t min_chunk) {
    // HK_STAGE_CHUNK_KB: chunk size for tests of the chunked paths (default 8 MB; never below one device row)
    static const size_t chunk_min = cap_from_env("HK_STAGE_CHUNK_KB", STAGE_CHUNK_MIN);
    const size_t want = std::max(min_chunk, chunk_min);
    if (s.stage && s.stage_chunk >= want) return HK_OK;
    int rc = stage_drain(s);
    if (rc) return rc;
    if (s.stage) HK_HIP(hipHostFree(s.stage));
    s.stage = nullptr, s.stage_chunk = 0;
    const size_t chunk = (want + 4095) / 4096 * 4096;
    if (hipHostMalloc(reinterpret_cast<void**>(&s.stage), chunk * Slot::STAGE_N, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        s.stage = nullptr;
        return fail(HK_ERR_NOMEM, "hipHostMalloc(%zu) failed", chunk * Slot::STAGE_N);
    }
    s.stage_chunk = chunk;
    for (int i = 0; i < Slot::STAGE_N; ++i)
        if (!s.stage_ev[i]) HK_HIP(hipEventCreateWithFlags(&s.stage_ev[i], hipEventDisableTiming));
    return HK_OK;
}

int stage_take(Slot& s, int* chunk) {
    g_staged_chunks.fetch_add(1, std::memory_order_relaxed);
    const int i = s.stage_next;
    s.stage_next = (s.stage_next + 1) % Slot::STAGE_N;
    const int rc = stage_settle(s, i);
    *chunk = i;
    return rc;
}

// `rows` rows of `row_bytes` from the host (rows h_pitch bytes apart) to the device (rows d_pitch bytes apart), queued on the
// slot's stream.  The host side may be released when the call returns (pageable memory: it has been packed; page-locked
// memory: the caller keeps it until the stream has been synchronised, as the entry points do before they return).
// The reverse (TO_DEVICE false): the caller's array is final after stage_drain() (pageable) / after the stream has been
// synchronised (pinned).  One body for both directions; only the side that is written differs.
template <bool TO_DEVICE>
int stage_copy(Slot& s, char* d, size_t d_pitch, char* h, size_t h_pitch, size_t row_bytes, size_t rows) {
    constexpr hipMemcpyKind kind = TO_DEVICE ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    if (rows == 0 || row_bytes == 0) return HK_OK;
    if (rows == 1) h_pitch = d_pitch = row_bytes;
    const bool flat = h_pitch == row_bytes && d_pitch == row_bytes;
    if (host_is_pinned(h, (rows - 1) * h_pitch + row_bytes)) {
        if (assert_pinned_on()) {
            const int rc = check_rows_pinned(h, h_pitch, row_bytes, rows);
            if (rc) return rc;
        }
        g_direct_copies.fetch_add(1, std::memory_order_relaxed);
        s.direct_pending = true;
        if (flat) HK_HIP(hipMemcpyAsync(TO_DEVICE ? d : h, TO_DEVICE ? h : d, rows * row_bytes, kind, s.stream));
        else
            HK_HIP(hipMemcpy2DAsync(TO_DEVICE ? d : h, TO_DEVICE ? d_pitch : h_pitch, TO_DEVICE ? h : d, TO_DEVICE ? h_pitch : d_pitch,
                                    row_bytes, rows, kind, s.stream));
        return HK_OK;
    }
    int rc = ensure_stage(s, flat ? 0 : d_pitch);
    if (rc) return rc;
    // one chunk of the ring: `n` rows of `rb` bytes, c_pitch apart in the chunk and on the device (ONE contiguous copy), hp apart
    // on the host -- packed here on the way to the device, unpacked by stage_settle() on the way back
    auto chunk = [&s](char* dc, char* hc, size_t hp, size_t c_pitch, size_t rb, size_t n) -> int {
        int i;
        const int rc = stage_take(s, &i);
        if (rc) return rc;
        char* c = s.stage + (size_t)i * s.stage_chunk;
        if (TO_DEVICE)
            for (size_t r = 0; r < n; ++r) memcpy(c + r * c_pitch, hc + r * hp, rb);
        HK_HIP(hipMemcpyAsync(TO_DEVICE ? dc : c, TO_DEVICE ? c : dc, (n - 1) * c_pitch + rb, kind, s.stream));
        HK_HIP(hipEventRecord(s.stage_ev[i], s.stream));
        s.stage_state[i] = TO_DEVICE ? 1 : 2;
        if (!TO_DEVICE) s.stage_out[i] = {.h_dst = hc, .h_pitch = hp, .row_bytes = rb, .c_pitch = c_pitch, .rows = n};
        return HK_OK;
    };
    if (flat) {  // a byte stream: every chunk is one row of up to stage_chunk bytes
        const size_t total = rows * row_bytes;
        for (size_t off = 0; off < total; off += s.stage_chunk) {
            const size_t n = std::min(s.stage_chunk, total - off);
            if ((rc = chunk(d + off, h + off, n, n, n, 1))) return rc;
        }
        return HK_OK;
    }
    // packed at the DEVICE pitch: the chunk maps onto the device rows with one contiguous copy (the padding between two
    // rows travels along; it belongs to the plane and nobody reads it)
    const size_t per = std::max<size_t>(s.stage_chunk / d_pitch, 1);
    for (size_t r0 = 0; r0 < rows; r0 += per)
        if ((rc = chunk(d + r0 * d_pitch, h + r0 * h_pitch, h_pitch, d_pitch, row_bytes, std::min(per, rows - r0)))) return rc;
    return HK_OK;
}
int stage_h2d(Slot& s, void* d_dst, size_t d_pitch, const void* h_src, size_t h_pitch, size_t row_bytes, size_t rows) {
    return stage_copy<true>(s, static_cast<char*>(d_dst), d_pitch, const_cast<char*>(static_cast<const char*>(h_src)), h_pitch, row_bytes, rows);
}
int stage_d2h(Slot& s, void* h_dst, size_t h_pitch, const void* d_src, size_t d_pitch, size_t row_bytes, size_t rows) {
    return stage_copy<false>(s, const_cast<char*>(static_cast<const char*>(d_src)), d_pitch, static_cast<char*>(h_dst), h_pitch, row_bytes, rows);
}

// A host-pointer call is ending WITHOUT stage_finish (an error return somewhere behind a stage_d2h): its queued chunks still name
// the caller's output arrays, which the caller may free as soon as it sees the error -- the next call on this slot must not unpack
// into them.  Let the copies that were queued complete (they write the ring, never the caller) and forget them.  The same goes for
// DIRECT copies (page-locked caller arrays, the RasterFuse default): they are still in flight on the caller's memory, which the
// caller may unregister and free once it has the error -- the stream is drained before the call returns (round-5 advisor finding).
void stage_abandon(Slot& s) {
    bool any = s.direct_pending;
    for (int i = 0; i < Slot::STAGE_N; ++i) any |= s.stage_state[i] != 0;
    if (!any) return;
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    (void)hipGetLastError();
    for (int i = 0; i < Slot::STAGE_N; ++i) s.stage_state[i] = 0;
    s.direct_pending = false;
}

// end of a host-pointer call: everything queued on the slot's stream has run and every output array is final
int stage_finish(Slot& s) {
    const int rc = stage_drain(s);
    if (rc) return rc;
    HK_HIP(hipStreamSynchronize(s.stream));
    s.direct_pending = false;
    return HK_OK;
}

// One plane of a caller's host raster: rows `stride` elements apart
struct HostGrid {
    const void* data;
    int64_t stride;
    int32_t height, width;
};

// A host raster into the float32 device plane `dplane` (row stride `dstride` elements): float32 directly, other dtypes through
// the raw plane `raw` (the same stride, in elements of the dtype) and the on-device conversion
int stage_in(Slot& s, const HostGrid& g, int dt, float* dplane, void* raw, int64_t dstride) {
    const size_t es = hk::dtype_size(dt);
    void* dst = dt ? raw : static_cast<void*>(dplane);
    const int rc = stage_h2d(s, dst, dstride * es, g.data, g.stride * es, (size_t)g.width * es, g.height);
    if (rc) return rc;
    if (dt)
        HK_HIP(hk::launch_cast_in(dt, {.in = dst, .in_stride = dstride, .out = dplane, .out_stride = dstride, .height = g.height,
                                       .width = g.width}, s.stream));
    return HK_OK;
}

void slot_release(Slot& s) {
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.dev) (void)dev_free(s.dev);
    if (s.norm_ws) (void)dev_free(s.norm_ws);
    if (s.aux) (void)dev_free(s.aux);
    if (s.comm_xchg) (void)dev_free(s.comm_xchg);
    if (s.open_rows) (void)dev_free(s.open_rows);
    if (s.fail_host) (void)hipHostFree(s.fail_host);
    if (s.stage) (void)hipHostFree(s.stage);
    for (int i = 0; i < Slot::STAGE_N; ++i)
        if (s.stage_ev[i]) (void)hipEventDestroy(s.stage_ev[i]);
    for (int i = 0; i < Slot::TBL_RING; ++i) {
        if (s.tbl_host[i]) (void)hipHostFree(s.tbl_host[i]);
        if (s.tbl_dev[i]) (void)dev_free(s.tbl_dev[i]);
        if (s.tbl_ev[i]) (void)hipEventDestroy(s.tbl_ev[i]);
    }
    if (s.stream) (void)hipStreamDestroy(s.stream);
    s = Slot();
}

// rasterio.enums.Resampling values with a device kernel (hk_resample.hip)
bool resampling_built(int m) { return (m >= 0 && m <= 6) || (m >= 8 && m <= 14); }  // all of GRA_* but gauss (7: not a warp method)

bool needs_r2(const hk_fit_desc* d) {
    return d->find_r2 || (d->model == HK_MODEL_GAIN_OFFSET && d->has_r2_thresh);
}

int validate_desc(const hk_fit_desc* d) {
    if (!d) return fail(HK_ERR_ARG, "desc is NULL");
    if (d->model < 0 || d->model > 2) return fail(HK_ERR_ARG, "unknown model %d", d->model);
    // homonim/utils.py:121-132
    if (d->kh < 1 || d->kw < 1) return fail(HK_ERR_ARG, "`kernel_shape` must be a minimum of one in both dimensions.");
    if ((d->kh & 1) == 0 || (d->kw & 1) == 0) return fail(HK_ERR_ARG, "`kernel_shape` must be odd in both dimensions.");
    if (d->model == HK_MODEL_GAIN_OFFSET && d->kh * d->kw < 2)
        return fail(HK_ERR_ARG, "`kernel_shape` area should contain at least 2 elements for the gain-offset model.");
    if (d->kh > 255) return fail(HK_ERR_UNSUPPORTED, "kernel height %d > 255 not supported", d->kh);
    if (hk::overlap_lanes_for(d->kw / 2) > 24) return fail(HK_ERR_UNSUPPORTED, "kernel width %d too large", d->kw);
    return check_nodata_modes(d->src_nodata_mode, d->ref_nodata_mode);
}

// RasterArray._convert_array_dtype refuses an output nodata that does not survive the cast to the output dtype
// (raster_array.py:357-358, rasterio.dtypes.can_cast_dtype); cast_out_kernel converts it with `(T)nodata`, which is undefined for
// a value the type cannot hold.  Integer types: an integer of the type's range (NaN and +-inf are none); float32: anything that
// does not overflow it (can_cast_dtype compares floats with np.allclose); float64: anything.  `dtype` is a valid hk_dtype.
// int_sample_holds: is `v` a value of the integer sample type `dtype` (NaN and +-inf fail both comparisons)?
bool int_sample_holds(int dtype, double v) {
    static const double lo[7] = {0, 0, 0, -32768.0, 0, -2147483648.0, 0}, hi[7] = {0, 255.0, 65535.0, 32767.0, 4294967295.0, 2147483647.0, 0};
    return v >= lo[dtype] && v <= hi[dtype] && v == std::floor(v);
}
int validate_out_nodata(int dtype, int has_nodata, double nodata) {
    if (!has_nodata || dtype == HK_DTYPE_F64) return HK_OK;
    static const char* const names[7] = {"float32", "uint8", "uint16", "int16", "uint32", "int32", "float64"};
    // float32: below the midpoint of FLT_MAX and 2^128
    const bool ok = dtype == HK_DTYPE_F32 ? !std::isfinite(nodata) || std::fabs(nodata) < 0x1.ffffffp127 : int_sample_holds(dtype, nodata);
    if (!ok) return fail(HK_ERR_ARG, "'nodata' value: %.17g cannot be safely cast to '%s'", nodata, names[dtype]);
    return HK_OK;
}

// The reference decides `(1 - f32(f64(ssres / sstot))) > thresh` (kernel_model.py:212-213,363).  Returns a float64 factor
// c such that, for sstot > 0, `ssres < c * sstot` PROVES that decision true: c sits 2^-40 (relative) below the
// float32 rounding boundary of the largest quotient that still passes, which swallows the 2^-53 errors of the float64
// division and of the comparison product.  -inf = nothing can be certified (threshold >= 1 or NaN).
double r2_pass_scale(float thresh) {
    if (!(thresh < 1.0f)) return -INFINITY;
    // largest float q with (1.0f - q) > thresh: the predicate is monotone non-increasing in q
    auto key = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); };
    auto unkey = [](uint32_t k) { uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; float f; memcpy(&f, &u, 4); return f; };
    uint32_t lo = key(-FLT_MAX), hi = key(FLT_MAX);  // pred(lo) is true for every thresh < 1
    auto pred = [&](uint32_t k) { volatile float d = 1.0f - unkey(k); return d > thresh; };
    if (!pred(lo)) return -INFINITY;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (pred(mid)) lo = mid; else hi = mid - 1;
    }
    const float q = unkey(lo);
    const float qn = nextafterf(q, INFINITY);
    const double boundary = std::isinf(qn) ? (double)q : 0.5 * ((double)q + (double)qn);
    if (!(boundary > 0.0)) return -INFINITY;
    return boundary * (1.0 - 0x1p-40);
}

// The mirror image: for sstot > 0, `ssres > c_hi * sstot` PROVES the decision false (c_hi sits 2^-40 above the same
// rounding boundary).  +inf = failure is never certified (degenerate thresholds): the division decides.
double r2_fail_above(float thresh) {
    const double c = r2_pass_scale(thresh);
    if (!(c > 0.0)) return INFINITY;
    return c / (1.0 - 0x1p-40) * (1.0 + 0x1p-40);
}

// kappa >= 1 - c' with c' = c * (1 - 2^-50) (so that `ssres < c' * sstot` in real arithmetic implies the float64
// comparison against fl(c * sstot)), clamped to >= 0 and rounded up to float32.  +inf = nothing can be certified.
float r2_fail_scale(float thresh) {
    const double c = r2_pass_scale(thresh);
    if (!(c > 0.0)) return INFINITY;
    double k = 1.0 - c * (1.0 - 0x1p-50);
    if (k < 0.0) k = 0.0;
    float kf = (float)k;
    if ((double)kf < k + 0x1p-60) kf = nextafterf(kf, INFINITY);
    return kf;
}

// kappa_f <= 1 - c_hi * (1 + 2^-50) with c_hi = r2_fail_above(): `g^2 den < kappa_f * sstot - (rounding slack)` then gives
// ssres > c_hi * sstot in real arithmetic with room for the float64 comparison, i.e. the reference's decision is False
// (PROOFS.md appendix A, the fail side).  Rounded DOWN to float32; -inf = failure is never certified that way.
float r2_failcert_scale(float thresh) {
    const double c_hi = r2_fail_above(thresh);
    if (!(c_hi > 0.0) || std::isinf(c_hi)) return -INFINITY;
    const double k = 1.0 - c_hi * (1.0 + 0x1p-50);
    if (!(k > 0.0)) return -INFINITY;
    float kf = (float)k;
    if ((double)kf > k - 0x1p-60) kf = nextafterf(kf, -INFINITY);
    return kf;
}

// Fewer resident waves for the dense `gain` kernel on large rasters: at 8 KB of LDS per wave 20 waves per CU stream their rows
// at once and the HBM answers with ~5.0 TB/s; 4 KB of unused LDS per wave leave 12 (three lock-step workgroups per CU) and it
// answers with 5.4: gain 5x5 at 16384^2 x 4 2.58 -> 2.37 ms, configs[1] 0.631 -> 0.605 ms, 3x3 -2.5 % (profiles/r03_lds_pad.txt).
// Not for the general (nodata) build -- its registers keep it at that occupancy already --, not for 7x7 (12 KB ring), not for
// launches of less than ~128 M pixels (a 4-band 4096^2 tile: +3 %); the VALU-bound builds want every wave (headline +8 % at 16
// -> 14 waves).  lds_pad_by_size: the build takes the pad by the launch's size, lds_pad_of: the pad for that many pixels.
bool lds_pad_by_size(const hk_fit_desc* d, const LaunchPolicy& lp) {
    return d->model == HK_MODEL_GAIN && !needs_r2(d) && d->kh <= 5 && d->kw <= 7 && d->src_nodata_mode == HK_NODATA_NONE &&
           d->ref_nodata_mode == HK_NODATA_NONE && !lp.force_general;
}
int lds_pad_of(long long pixels) { return pixels >= (128ll << 20) ? 4096 : 0; }

void fill_args(hk::FitArgs& a, const hk_fit_desc* d, const LaunchPolicy& lp) {
    a.rh = d->kh / 2;
    a.rw = d->kw / 2;
    a.overlap_lanes = hk::overlap_lanes_for(a.rw);
    a.src_nd_mode = d->src_nodata_mode;
    a.ref_nd_mode = d->ref_nodata_mode;
    a.src_nodata = d->src_nodata;
    a.ref_nodata = d->ref_nodata;
    a.has_thresh = (d->model == HK_MODEL_GAIN_OFFSET) ? d->has_r2_thresh : 0;
    a.r2_thresh = d->r2_thresh;
    a.r2_fail_scale = a.has_thresh ? r2_fail_scale(d->r2_thresh) : INFINITY;
    a.r2_failcert_scale = a.has_thresh ? r2_failcert_scale(d->r2_thresh) : -INFINITY;
    a.r2_pass_below = a.has_thresh ? r2_pass_scale(d->r2_thresh) : -INFINITY;
    a.r2_fail_above = a.has_thresh ? r2_fail_above(d->r2_thresh) : INFINITY;
    a.n_full = (float)(d->kh * d->kw);
    a.nd_full = (double)(d->kh * d->kw);
    a.inv_n_full = 1.0 / (double)(d->kh * d->kw);
    a.force_general = lp.force_general;
    // ring mode (hk_fit_kernel.h): full LDS ring while it leaves room for >= 11 waves per CU (kh <= 5), centre-only ring up
    // to kh = 39 (1 KB per wave and row of the half-height; 33 - 39 rows: 3 - 13 % faster than re-loading, from 41 rows
    // slower -- headline workload, round 5), everything re-loaded beyond -- that path exists
    // for kernels from 9 wide only (hk_kernels.h fit_build_exists), narrower ones keep the centre ring whatever their height (kh <= 255: 128 KB)
    a.use_ring = (d->kh <= 5 && d->kw <= 7) ? 1 : ((d->kh <= 39 || d->kw <= 7) ? 2 : 0);
    // The memory-bound builds (no R2) prefer the full ring well beyond that: re-loading the leaving rows costs them more than
    // the waves the ring displaces -- gain 7x7 / 9x9 / 11x11 / 15x15 at 16384^2 x 4: 3.25 / 3.40 / 3.45 / 3.95 -> 2.54 / 2.58 /
    // 2.77 / 3.64 ms; gain-blk-offset (more arithmetic per pixel) only up to 7x7 (fit + statistics 5.11 -> 4.61 ms; 9x9 equal,
    // 15x15 +21 %)
    if (!needs_r2(d) && d->kw <= 15) {
        if (d->model == HK_MODEL_GAIN && d->kh <= 15) a.use_ring = 1;
        if (d->model == HK_MODEL_GAIN_BLK_OFFSET && d->kh <= 7 && d->kw <= 7) a.use_ring = 1;
        // Round 3, the SPLIT ring (rh rows in registers + rh + 1 in LDS: no re-load, 16 instead of 30 KB of LDS at 15x15):
        // gain 11x11 / 13x13 / 15x15 at 16384^2 x 4: 2.77 / 3.08 / 3.47 -> 2.70 / 2.86 / 3.07 ms (7x7 and 9x9 stay with the
        // full ring: 2.36 / 2.45 against 2.48 / 2.72); gain-blk-offset incl. statistics 9x9 / 11x11: 5.23 / 5.38 -> 4.95 /
        // 5.27 ms -- but 13x13 / 15x15 get SLOWER (5.37 / 5.35 -> 5.57 / 5.99): with its float64 normalisation and quotient
        // per pixel and the 15-wide horizontal sums that kernel is bound by VALU issue, not by the 8 B per pixel the
        // re-load moves (profiles/r03_sweep_ring.txt).
        if (d->kw >= 5) {
            if (d->model == HK_MODEL_GAIN && d->kh >= 11 && d->kh <= 15) a.use_ring = 3;
            if (d->model == HK_MODEL_GAIN_BLK_OFFSET && d->kh >= 9 && d->kh <= 11) a.use_ring = 3;
        }
    }
    // ... and, in their lock-step workgroups (hk_fit_kernel.h WPB), short uniform segments: 32 rows instead of 64 / 128 + 32
    // (gain 5x5: configs[1] 0.676 -> 0.625 ms, 16384^2 x 4 2.65 -> 2.49 ms on one box; 7x7 2.54 -> 2.47; gain-blk-offset 5x5
    // -0.5 %).  16 rows are as good or better at 5x5 but load a quarter more rows; taller kernels keep the default.
    a.seg_rows_pref = 0;
    if (!needs_r2(d) && a.use_ring == 1 && d->model != HK_MODEL_GAIN_OFFSET &&
        (d->kh <= 5 || (d->model == HK_MODEL_GAIN && d->kh <= 7)))
        a.seg_rows_pref = 32;
    if (lp.use_ring) {
        const int m = *lp.use_ring;
        const bool mem_bound = d->model != HK_MODEL_GAIN_OFFSET && !needs_r2(d);
        if (m == 1 && d->kh <= 63 && (d->kw <= 7 || (mem_bound && d->kw <= 15))) a.use_ring = 1;
        if (m == 2 && d->kh <= 127) a.use_ring = 2;
        if (m == 3 && mem_bound && d->kh >= 7 && d->kh / 2 <= hk::split_ring_rows(d->model) && d->kw >= 5 && d->kw <= 15) a.use_ring = 3;
        if (m == 0 && d->kw >= 9) a.use_ring = 0;
    }
    a.xcd_remap = lp.xcd_remap;
    a.lds_pad = lds_pad_by_size(d, lp) ? -1 : 0;  // -1 = decided by fill_grid() from the job's size
    a.out_y0 = 0, a.out_y1 = a.height, a.out_x0 = 0, a.out_x1 = a.width;  // store window: the whole job (callers narrow it)
}

// Row segments of the units (segment, band, strip), one wave each.  A wave re-reads 2*rh priming rows, so long segments waste
// less; but a launch ends when its last wave does, so its final segments are short.  A launch of at least `two_size_from`
// units therefore gets `big` rows per segment for most of its units and `tail` rows for those of its last `tail_waves` waves
// (dispatched last); smaller launches and an explicit height use `uniform` rows throughout.  fill_grid applies this over the
// rows of one job, hk_fit_apply_batch_dev over the jobs of a batched launch.
struct SegPolicy {
    int uniform;
    int big, tail;
    long long two_size_from;  // 6 generations of resident waves
    double tail_waves;        // the last 1.25 generations
};
SegPolicy seg_policy(int kh, const LaunchPolicy& lp) {
    const int uniform = kh <= 5 ? 64 : (kh <= 9 ? 128 : 256);
    const long long slots = lp.wave_slots;
    return {uniform, lp.seg_big.value_or(2 * uniform), lp.seg_tail.value_or(uniform / 2), 6 * slots, 1.25 * (double)slots};
}

// The units of one launch (fill_args done).  `seg_rows` > 0: segments of that height; otherwise the build's own preference
// (fill_args) or seg_policy().
void fill_grid(hk::FitArgs& a, int seg_rows, const LaunchPolicy& lp) {
    const int out_w = (hk::WAVE - 2 * a.overlap_lanes) * hk::PX;
    const SegPolicy seg = seg_policy(2 * a.rh + 1, lp);
    a.n_strips = (a.width + out_w - 1) / out_w;
    if (seg_rows <= 0 && a.seg_rows_pref > 0) seg_rows = a.seg_rows_pref;
    const int uniform = seg_rows > 0 ? seg_rows : seg.uniform;
    a.seg_rows = uniform < a.height ? uniform : a.height;
    a.seg_rows_tail = a.seg_rows;
    a.n_segs = (a.height + a.seg_rows - 1) / a.seg_rows;
    a.n_segs_big = a.n_segs;
    const long long per_row_band = (long long)a.n_strips * a.n_bands;  // units per segment row
    if (seg_rows <= 0 && per_row_band * a.n_segs >= seg.two_size_from) {
        const int big = seg.big, tail = seg.tail;
        // image rows whose big-segment units make up the tail's waves
        long long tail_rows = (long long)(seg.tail_waves / (double)per_row_band * big);
        tail_rows = (tail_rows + tail - 1) / tail * tail;
        if (big > 0 && tail > 0 && tail_rows < a.height - big) {
            const int n_big = (int)((a.height - tail_rows) / big);
            const int rest = a.height - n_big * big;
            a.seg_rows = big;
            a.seg_rows_tail = tail;
            a.n_segs_big = n_big;
            a.n_segs = n_big + (rest + tail - 1) / tail;
        }
    }
    a.total_units = a.n_strips * a.n_segs * a.n_bands;
    if (a.lds_pad < 0) a.lds_pad = lds_pad_of((long long)a.height * a.width * a.n_bands);
}

// The slot's scratch of the in-painting branch for a height x stride plane, [offset plane | workspace of launch_inpaint_offsets]:
// the one place that knows it.  Grows sl.aux as needed (which lock covers that is the caller's business).  Rows are padded
// to quads (stride % 4 == 0), so the workspace's base is 16-byte aligned behind the plane.
struct InpaintScratch {
    float* offset;        // an offset plane for a pass whose caller keeps none
    unsigned char* flag;  // the workspace's source-flag plane, for a fit to write (FitArgs::flag)
    void* ws;             // the workspace
};
static int inpaint_scratch(Slot& sl, int height, long long stride, InpaintScratch& s) {
    const size_t plane = (size_t)stride * height * sizeof(float);
    const int rc = grow_slot_buf(sl, sl.aux, sl.aux_bytes, plane + hk::inpaint_workspace_bytes(height, stride));
    if (rc) return rc;
    s.offset = static_cast<float*>(sl.aux);
    s.ws = static_cast<char*>(sl.aux) + plane;
    s.flag = hk::inpaint_flag_plane(s.ws, height, stride);
    return HK_OK;
}
// What the in-painting of a band reads, where a pass has left it ready: the offsets and the source flags (r2 > thresh) & (gain > 0)
// & valid that the fused kernel writes beside them (FitArgs::flag)
struct InpaintInputs {
    float* offset;
    const unsigned char* flag;
};

// gain-offset with the r2 mask when nothing but the corrected block (and, from scratch, the offsets) is asked for and the failures
// are counted: the CERTIFICATE build runs first (118 - 126 registers, four waves per SIMD: the division-free float32 certificate of
// PROOFS.md appendix A settles a wave-row whose every valid pixel certainly passes) and marks the wave-rows it cannot settle in
// a bit plane; the LIST launch -- the complete build on a persistent grid, one run of marked rows per wave at a time -- follows on
// the same stream and does those rows with the reference's own R2 expression.  Together they write every row once and count every
// failing pixel once; an empty bit plane (clean rasters) costs the list launch a few microseconds.  (The certificate has builds for
// the full and the centre ring, its constants assume window counts below 2^16, and the in-painting's source flags do not fit its
// registers: other shapes, R2 / gain output and launches that leave the in-painting's inputs run the complete build over the
// whole grid: hk::choose_fit_build says which.)
static bool cert_list_eligible(hk::FitArgs a, const hk_fit_desc* desc, bool r2) {
    a.cert_only = 1, a.list_mode = 0;
    const bool cert = hk::fit_build_exists(hk::choose_fit_build(a, desc->model, r2));
    a.cert_only = 0, a.list_mode = 1;
    return cert && hk::fit_build_exists(hk::choose_fit_build(a, desc->model, r2));
}

// the fused launch of one job (fill_args + fill_grid done): certificate build + list launch where they apply, the one build otherwise
static int launch_fit(hk_ctx* ctx, Slot& sl, hk::FitArgs& a, const hk_fit_desc* desc, bool r2) {
    a.cert_only = 0, a.open_rows = nullptr, a.list_mode = 0;
    if (!cert_list_eligible(a, desc, r2)) {
        HK_HIP(hk::launch_fit_apply(a, desc->model, r2, sl.stream));
        return HK_OK;
    }
    const size_t bytes = (size_t)a.n_bands * (size_t)a.n_strips * (size_t)((a.height + 31) / 32) * sizeof(unsigned);
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        const int rc = grow_slot_buf(sl, sl.open_rows, sl.open_rows_bytes, bytes);
        if (rc) return rc;
    }
    hk::FitArgs c = a;
    c.open_rows = sl.open_rows;
    HK_HIP(hipMemsetAsync(c.open_rows, 0, bytes, sl.stream));
    c.cert_only = 1;
    HK_HIP(hk::launch_fit_apply(c, desc->model, r2, sl.stream));
    c.cert_only = 0, c.list_mode = 1;
    HK_HIP(hk::launch_fit_apply(c, desc->model, r2, sl.stream));
    return HK_OK;
}

// kernel_model.py:364-371 for ONE band whose first pass counted failing pixels: in-paint the offsets of the failing
// pixels from the passing ones (restated GDALFillNodata) and run the fit again with `offset_in`, which recomputes their
// gains and re-applies.  `a` is the first pass's argument block (n_bands == 1).
// `n_fail`: the band's r2-mask failure count.  `ready` (nullable): the in-painting's inputs as the pass that counted the failures
// left them -- the in-painting then starts right away.  `drop_params`: the parameter planes in `a` are scratch, the closing pass
// need not write them.
static int inpaint_band(Slot& sl, const hk::FitArgs& a, const hk_fit_desc* desc, bool r2, unsigned long long n_fail,
                        const InpaintInputs* ready, bool drop_params = false) {
    InpaintScratch s;
    {
        const int rc = inpaint_scratch(sl, a.height, a.stride, s);
        if (rc) return rc;
    }
    const hipStream_t stream = sl.stream;
    InpaintInputs in = {a.offset, nullptr};  // the caller's own planes: the in-painting makes the flags from gain / r2
    if (ready) {
        in = *ready;
    } else if (!a.gain || !a.offset || !a.r2) {
        // parameters were not materialised by the first pass: run it again for what the in-painting reads -- the offsets
        // and the source flags, which the kernel writes itself (1 byte per pixel)
        hk::FitArgs b = a;
        b.gain = nullptr, b.r2 = nullptr, b.offset = s.offset, b.corr = nullptr, b.fail_count = nullptr;
        b.flag = s.flag;
        b.cert_only = 0, b.open_rows = nullptr, b.list_mode = 0;
        HK_HIP(hk::launch_fit_apply(b, desc->model, r2, stream));
        in = {s.offset, s.flag};  // the slot's scratch, written by the pass just queued
    }
    // The failing pixels' offsets are in-painted IN PLACE (round 5; a separate `filled` plane cost a pass-through of every source
    // pixel): sources are read only where the flag is 1, targets written only where it is 0, and the closing pass -- which reads the
    // plane at the failing pixels only -- rewrites the caller's offset plane whole when there is one.
    hk::InpaintArgs ia;
    ia.offset = in.offset, ia.stride = a.stride, ia.height = a.height, ia.width = a.width;
    ia.flag_ready = in.flag, ia.gain = a.gain, ia.r2 = a.r2, ia.thresh = desc->r2_thresh;
    ia.n_targets = n_fail;
    HK_HIP(hk::launch_inpaint_offsets(ia, s.ws, stream));
    // closing pass: the failing pixels take the in-painted offsets and recomputed gains (kernel_model.py:370-371).  Which
    // pixels failed is in the flag plane the in-painting just used, so the build WITHOUT the R2 work runs (the R2 plane, if
    // the caller keeps one, was written by the pass that counted and is not changed by the branch)
    hk::FitArgs c = a;
    c.offset_in = in.offset;
    c.flag_in = in.flag ? in.flag : s.flag;
    c.fail_count = nullptr;  // already counted
    c.flag = nullptr;
    c.r2 = nullptr;
    c.cert_only = 0, c.open_rows = nullptr, c.list_mode = 0;
    if (drop_params) c.gain = c.offset = nullptr;  // nobody reads them after this
    HK_HIP(hk::launch_fit_apply(c, desc->model, false, stream));
    return HK_OK;
}

// The fused kernel's argument block for a device-resident job, or for band `band` of it alone: its planes, shape and store
// window, the build's launch policy (fill_args) and its units (fill_grid with the job's seg_rows).
int job_fit_args(hk::FitArgs& a, const hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job& job, int band = -1) {
    const int b = band < 0 ? 0 : band;
    const long long off = (long long)b * job.band_stride;
    auto plane = [off](float* p) { return p ? p + off : nullptr; };
    memset(&a, 0, sizeof(a));
    a.src = job.src + off, a.ref = job.ref + off;
    a.gain = plane(job.gain), a.offset = plane(job.offset), a.r2 = plane(job.r2), a.corr = plane(job.corr);
    a.norm = job.norm ? job.norm + 2 * b : nullptr;
    a.fail_count = job.fail_count ? reinterpret_cast<unsigned long long*>(job.fail_count) + b : nullptr;
    a.height = job.height, a.width = job.width, a.stride = job.stride;
    a.band_stride = band < 0 ? job.band_stride : 0;
    a.n_bands = band < 0 ? job.n_bands : 1;
    fill_args(a, desc, ctx->launch);
    fill_grid(a, job.seg_rows, ctx->launch);
    if (job.out_rows || job.out_cols) {  // the halo crop of a block processed in place inside a larger raster
        if (a.has_thresh)
            return fail(HK_ERR_UNSUPPORTED, "a store window is not supported together with r2_inpaint_thresh (the in-painting "
                                            "needs the parameters of the whole block)");
        a.out_y0 = job.out_row0, a.out_y1 = job.out_row0 + job.out_rows;
        a.out_x0 = job.out_col0, a.out_x1 = job.out_col0 + job.out_cols;
    }
    return HK_OK;
}

// The block statistics' argument block (gain-blk-offset) for n_bands planes src / ref + band * band_stride
hk::NormArgs norm_args(const hk_fit_desc* desc, const float* src, const float* ref, int height, int width, long long stride,
                       long long band_stride = 0, int n_bands = 1) {
    hk::NormArgs na;
    na.src = src, na.ref = ref, na.height = height, na.width = width, na.stride = stride;
    na.band_stride = band_stride, na.n_bands = n_bands;
    na.src_nd_mode = desc->src_nodata_mode, na.ref_nd_mode = desc->ref_nodata_mode;
    na.src_nodata = desc->src_nodata, na.ref_nodata = desc->ref_nodata;
    return na;
}

// A fit whose r2-mask outcome has not been looked at yet (run_host reads the counter together with the outputs: one
// stream synchronisation per block when no pixel fails, which is the usual case on well-conditioned imagery)
struct FitPending {
    hk::FitArgs a;
    bool scratch_params = false;  // a.offset / a.flag are the slot's scratch (written for the in-painting only)
    bool active = false;  // gain-offset with a threshold: fit_finish() has to look at the counter
};

// second half of fit_on_device, once the failure counter is on the host: the in-painting branch (kernel_model.py:361-371).  *requeued = the output planes were (re)written by work queued here.
int fit_finish(hk_ctx* ctx, Slot& sl, const hk_fit_desc* desc, FitPending& p, unsigned long long n_fail, bool* requeued) {
    *requeued = false;
    if (!p.active) return HK_OK;
    hk::FitArgs& a = p.a;
    const bool r2 = needs_r2(desc);
    ctx->expect_r2_failures.store(n_fail > 0 ? 1 : 0);
    if (n_fail > 0) {
        const InpaintInputs first_pass = {a.offset, a.flag};  // written by fit_on_device's pass where it expected failures (a.flag set)
        const int rc = inpaint_band(sl, a, desc, r2, n_fail, a.flag ? &first_pass : nullptr, p.scratch_params);
        if (rc) return rc;
        *requeued = true;
    }
    return HK_OK;
}

// Device-side KernelModel.fit (+ apply when job.corr) of one float32 block already in HBM: block statistics for
// gain-blk-offset (or the caller's norm), the fused kernel, and the in-painting branch of gain-offset
// (kernel_model.py:361-371) when valid pixels fail the r2 mask.  `job`: the block as a one-band job on the slot's stream --
// gain / offset / r2 / corr nullable; norm: two device words that receive the statistics here (used by gain-blk-offset only);
// fail_count: cleared here; out_row0 .. out_cols: the store window of the kernel, all zero = the whole block.
// `defer` (nullable): only queue the first pass and leave the r2-mask outcome to the caller (fit_finish); otherwise the
// stream is synchronised here to read the counter.
int fit_on_device(hk_ctx* ctx, Slot& sl, const hk_fit_desc* desc, hk_dev_job job, void* d_norm_ws, const double* norm_in = nullptr,
                  FitPending* defer = nullptr) {
    const bool blk = desc->model == HK_MODEL_GAIN_BLK_OFFSET;
    const bool r2 = needs_r2(desc);
    unsigned long long* const d_fail = reinterpret_cast<unsigned long long*>(job.fail_count);
    double* const d_norm = const_cast<double*>(job.norm);  // (the job's view of it is the kernel's: read-only)
    HK_HIP(hipMemsetAsync(d_fail, 0, sizeof(unsigned long long), sl.stream));
    if (!blk) {
        job.norm = nullptr;
    } else if (norm_in) {
        memcpy(sl.pin<double>(Slot::PIN_NORM_IN), norm_in, 2 * sizeof(double));  // (caller memory -> pinned words)
        HK_HIP(hipMemcpyAsync(d_norm, sl.pin<double>(Slot::PIN_NORM_IN), 2 * sizeof(double), hipMemcpyHostToDevice, sl.stream));
    } else {
        HK_HIP(hk::launch_block_norm(norm_args(desc, job.src, job.ref, job.height, job.width, job.stride), d_norm_ws, d_norm, sl.stream));
    }
    // the in-painting branch needs the parameters of the whole block: the store window only narrows the other models
    if (desc->model == HK_MODEL_GAIN_OFFSET && desc->has_r2_thresh) job.out_row0 = job.out_rows = job.out_col0 = job.out_cols = 0;
    FitPending local;
    FitPending& p = defer ? *defer : local;
    hk::FitArgs& a = p.a;
    int rc = job_fit_args(a, ctx, desc, job);
    if (rc) return rc;
    p.scratch_params = false;
    if (a.has_thresh && desc->model == HK_MODEL_GAIN_OFFSET && ctx->expect_r2_failures.load()) {
        // what the in-painting reads -- offsets and source flags -- into the slot's scratch right away: no second "first
        // pass" (fit_finish hands them to inpaint_band).  With the caller's own offset plane only the flags are scratch.
        InpaintScratch s;
        rc = inpaint_scratch(sl, job.height, job.stride, s);
        if (rc) return rc;
        a.flag = s.flag;
        if (!job.offset) {
            a.offset = s.offset;
            p.scratch_params = !job.gain && !job.r2;
        }
    }
    rc = launch_fit(ctx, sl, a, desc, r2);
    if (rc) return rc;
    p.active = a.has_thresh != 0;
    if (defer || !p.active) return HK_OK;

    // kernel_model.py:361-371: when valid pixels fail (r2 > thresh) & (gain > 0), in-paint their offsets from the
    // passing ones and recompute their gains.  Needs the count on the host (one extra stream sync per call).
    HK_HIP(hipMemcpyAsync(sl.fail_host, d_fail, sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    HK_HIP(hipStreamSynchronize(sl.stream));
    bool requeued = false;
    return fit_finish(ctx, sl, desc, p, *sl.fail_host, &requeued);
}

// What hk_io_desc (nullable: float32 everywhere) and the model say about a host-pointer fit's inputs and outputs
struct FitIo {
    int sdt = 0, rdt = 0, odt = 0, out_has_nodata = 0;
    double out_nodata = 0;
    bool out_cast = false, r2 = false;  // out_cast: the corrected plane goes through cast_out (another dtype, or an output nodata)
    bool want_valid = false;            // ... through cast_out_valid, which writes the validity plane beside it (float32 included)
};
int check_fit_io(const hk_fit_desc* desc, const hk_io_desc* io, const float* params_out, int32_t n_param_bands, FitIo* f,
                 const void* corr_out = nullptr, const uint8_t* valid_out = nullptr) {
    if (io) f->sdt = io->src_dtype, f->rdt = io->ref_dtype, f->odt = io->out_dtype;
    if (!hk::dtype_size(f->sdt) || !hk::dtype_size(f->rdt) || !hk::dtype_size(f->odt)) return fail(HK_ERR_ARG, "unknown dtype");
    if (io) {
        const int rc = validate_out_nodata(f->odt, io->out_has_nodata, io->out_nodata);
        if (rc) return rc;
        f->out_cast = f->odt != 0 || io->out_has_nodata;
        f->out_has_nodata = io->out_has_nodata, f->out_nodata = io->out_nodata;
    }
    if (valid_out) {
        if (!corr_out) return fail(HK_ERR_ARG, "valid_out needs corr_out: validity is that of the corrected block");
        f->want_valid = f->out_cast = true;
    }
    f->r2 = needs_r2(desc);
    if (params_out && n_param_bands != (f->r2 ? 3 : 2))
        return fail(HK_ERR_ARG, "n_param_bands must be %d for this model configuration", f->r2 ? 3 : 2);
    return HK_OK;
}

// the whole block of `rows` x `cols`, written packed
hk_out_window whole_block(int32_t rows, int32_t cols) { return {cols, (int64_t)rows * cols, 0, 0, rows, cols, cols}; }

// Where a host-pointer fit's results lie on the device and where they go in the caller's memory.  A window's param_stride is the
// row stride of params_out.
struct FitResults {
    float* params_out;        // nullable: n_param_bands planes, ...
    int32_t n_param_bands;
    const float* d_par;       // ... on the device d_par_band elements apart, rows d_par_stride apart, ...
    int64_t d_par_stride, d_par_band;
    hk_out_window pw;         // ... and their window into the caller's planes
    void* corr_out;           // nullable: the corrected plane, ...
    const float* d_corr;      // ... on the device height x width, rows d_stride apart, ...
    void* d_raw;              // ... through here and the cast where the output has one (FitIo::out_cast), ...
    int64_t d_stride;
    int32_t height, width;
    hk_out_window cw;         // ... and its window into corr_out
    uint8_t* valid_out = nullptr;        // nullable: the validity of the corrected plane (255 / 0), the same window and row stride, ...
    unsigned char* d_valid = nullptr;    // ... on the device rows d_stride bytes apart (FitIo::want_valid)
};
// The corrected plane as the output holds it: through the cast where the output has one (FitIo::out_cast), which writes the validity
// plane beside it (FitIo::want_valid).  *d_out: where the plane then lies, rows d_stride elements of the output dtype apart.
int cast_fit_results(Slot& sl, const FitIo& f, const FitResults& r, const char** d_out) {
    *d_out = reinterpret_cast<const char*>(r.d_corr);
    if (!f.out_cast) return HK_OK;
    const hk::CastPlane cp = {.in = r.d_corr, .in_stride = r.d_stride, .out = r.d_raw, .out_stride = r.d_stride,
                              .height = r.height, .width = r.width, .has_nodata = f.out_has_nodata, .nodata = f.out_nodata,
                              .valid = r.d_valid, .valid_stride = r.d_stride};
    HK_HIP(f.want_valid ? hk::launch_cast_out_valid(f.odt, cp, sl.stream) : hk::launch_cast_out(f.odt, cp, sl.stream));
    *d_out = static_cast<const char*>(r.d_raw);
    return HK_OK;
}
// queues the copies of both, and behind them the r2-mask failure counter (nullable d_fail) into the slot's pinned word
int stage_fit_results(Slot& sl, const FitIo& f, const FitResults& r, const unsigned long long* d_fail) {
    int rc;
    const hk_out_window &pw = r.pw, &cw = r.cw;
    if (r.params_out)
        for (int b = 0; b < r.n_param_bands; ++b)
            if ((rc = stage_d2h(sl, r.params_out + (size_t)b * pw.band_stride, pw.param_stride * sizeof(float),
                                r.d_par + (size_t)b * r.d_par_band + (size_t)pw.row0 * r.d_par_stride + pw.col0,
                                r.d_par_stride * sizeof(float), (size_t)pw.cols * sizeof(float), pw.rows)))
                return rc;
    if (r.corr_out) {
        const size_t es = hk::dtype_size(f.odt);  // (4 without a cast: the output is float32 then)
        const char* d_out;
        if ((rc = cast_fit_results(sl, f, r, &d_out))) return rc;
        if ((rc = stage_d2h(sl, r.corr_out, cw.stride * es, d_out + ((size_t)cw.row0 * r.d_stride + cw.col0) * es, r.d_stride * es,
                            (size_t)cw.cols * es, cw.rows)))
            return rc;
        if (f.want_valid &&
            (rc = stage_d2h(sl, r.valid_out, cw.stride, r.d_valid + (size_t)cw.row0 * r.d_stride + cw.col0, r.d_stride, cw.cols, cw.rows)))
            return rc;
    }
    if (d_fail) HK_HIP(hipMemcpyAsync(sl.fail_host, d_fail, sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    return HK_OK;
}
// The same results for a caller whose rasters are on the device (params_out, corr_out and valid_out are device pointers here): the
// windows go to their places by strided device copies, in stream order; valid_stride: bytes between the rows of valid_out.
int place_fit_results(Slot& sl, const FitIo& f, const FitResults& r, int64_t valid_stride) {
    int rc;
    const hk_out_window &pw = r.pw, &cw = r.cw;
    auto copy = [&](void* dst, size_t d_pitch, const void* src, size_t s_pitch, size_t row_bytes, size_t rows) {
        return hipMemcpy2DAsync(dst, d_pitch, src, s_pitch, row_bytes, rows, hipMemcpyDeviceToDevice, sl.stream);
    };
    if (r.params_out)
        for (int b = 0; b < r.n_param_bands; ++b)
            HK_HIP(copy(r.params_out + (int64_t)b * pw.band_stride, pw.param_stride * sizeof(float),
                        r.d_par + (int64_t)b * r.d_par_band + (int64_t)pw.row0 * r.d_par_stride + pw.col0,
                        r.d_par_stride * sizeof(float), (size_t)pw.cols * sizeof(float), pw.rows));
    if (r.corr_out) {
        const size_t es = hk::dtype_size(f.odt);
        const char* d_out;
        if ((rc = cast_fit_results(sl, f, r, &d_out))) return rc;
        HK_HIP(copy(r.corr_out, cw.stride * es, d_out + ((int64_t)cw.row0 * r.d_stride + cw.col0) * es, r.d_stride * es,
                    (size_t)cw.cols * es, cw.rows));
        if (f.want_valid)
            HK_HIP(copy(r.valid_out, valid_stride, r.d_valid + (int64_t)cw.row0 * r.d_stride + cw.col0, r.d_stride, cw.cols, cw.rows));
    }
    return HK_OK;
}

// mask_partial counts the valid pixels of a (kh+2) x (kw+2) window in an unsigned short (hk_mask.hip)
int check_mask_kernel(int kh, int kw) {
    return (kh + 2) * (kw + 2) > 65535 ? fail(HK_ERR_UNSUPPORTED, "kernel too large for mask_partial") : HK_OK;
}

// What hk_refspace_fit_apply and hk_srcspace_fit_apply ask alike of a source block and a reference block on another grid.
// (The mask_partial refusal cannot be reached today: validate_desc keeps kh <= 255 and kw <= 193, 257 * 195 counts fit.)
template <class Space, class Grid>
int check_two_grid_args(const hk_fit_desc* desc, const Space* space, const Grid& src, const Grid& ref, const void* corr_out) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    if (!space || !src.data || !ref.data || !corr_out) return null_arg();
    if (src.height < 1 || src.width < 1 || ref.height < 1 || ref.width < 1) return fail(HK_ERR_ARG, "empty raster");
    if ((rc = check_strides(src.stride, src.width, ref.stride, ref.width))) return rc;
    if (src.height > 65535 || ref.height > 65535) return fail(HK_ERR_UNSUPPORTED, "block taller than 65535 rows");
    return space->mask_partial ? check_mask_kernel(desc->kh, desc->kw) : HK_OK;
}
template <class Space>
int check_two_grids(const hk_ctx* ctx, const hk_fit_desc* desc, const Space* space, const HostGrid& src, const HostGrid& ref,
                    const void* corr_out) {
    return ctx ? check_two_grid_args(desc, space, src, ref, corr_out) : fail(HK_ERR_ARG, "ctx is NULL");
}

// hk_reproject and hk_reproject_dev ask the same of a re-projection between two axis-aligned grids of one CRS; the band count is
// gridDim.z of the launch.  `host_form`: hk_reproject's wording for a resampling that is not built.
int check_reproject(const hk_ctx* ctx, const hk::ResamplePlanes& p, double kx, double ky, int32_t resampling, bool host_form) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!p.src || !p.dst) return null_arg();
    if (p.n_bands < 1 || p.sh < 1 || p.sw < 1 || p.dh < 1 || p.dw < 1) return fail(HK_ERR_ARG, "empty raster");
    if (p.n_bands > 65535) return fail(HK_ERR_ARG, "too many bands for one launch (%d > 65535)", p.n_bands);
    if (!(kx > 0.0) || !(ky > 0.0)) return fail(HK_ERR_UNSUPPORTED, "flipped or degenerate grid mapping");
    if (!resampling_built(resampling))
        return fail(HK_ERR_UNSUPPORTED, host_form ? "resampling %d is not a warp method (GRA_* codes 0..6 and 8..14 are built; 7 = gauss is "
                                                    "an overview-only method in GDAL / rasterio as well)"
                                                  : "resampling %d is not a warp method", resampling);
    if (p.dh > 65535) return fail(HK_ERR_UNSUPPORTED, "destination taller than 65535 rows");
    return check_nodata_mode(p.nd_mode);
}
// ... and the device forms, whose planes carry strides, of those
int check_resample_strides(const hk::ResamplePlanes& p) {
    const int rc = check_strides(p.src_stride, p.sw, p.dst_stride, p.dw);
    return rc ? rc : check_band_strides(p.src_band_stride, p.dst_band_stride);
}

// The host form of a re-projection: `p` names the caller's packed arrays (its strides are not read).  The bands stay packed
// in the slab, the source at 0 and the destination behind it; `launch(planes, stream)` -> status runs on the slab's planes.
template <class Launch>
int reproject_packed(hk_ctx* ctx, const hk::ResamplePlanes& p, Launch launch) {
    HK_ENTER(ctx);
    const size_t sbytes = (size_t)p.n_bands * p.sh * p.sw * 4, dbytes = (size_t)p.n_bands * p.dh * p.dw * 4;
    const size_t o_dst = (sbytes + 255) / 256 * 256;
    HostCall hc(ctx, o_dst + dbytes);
    if (hc.rc) return hc.rc;
    hk::ResamplePlanes d = p;
    d.src = hc.at<float>(0), d.dst = hc.at<float>(o_dst);
    d.src_stride = p.sw, d.src_band_stride = (long long)p.sh * p.sw, d.dst_stride = p.dw, d.dst_band_stride = (long long)p.dh * p.dw;
    int rc = stage_h2d(hc.sl, hc.at(0), sbytes, p.src, sbytes, sbytes, 1);
    if (rc || (rc = launch(d, hc.sl.stream))) return rc;
    if ((rc = stage_d2h(hc.sl, p.dst, dbytes, d.dst, dbytes, dbytes, 1))) return rc;
    return stage_finish(hc.sl);
}

// A host-pointer fit as its entry point received it: one source and one reference block of height x width on the same grid.
// `corr_out` / `params_out` nullable; `window` nullable: the window of the block that is written to corr_out / params_out and
// their row / plane strides (hk_out_window), else the whole block, packed.
struct HostFit {
    const void* src;
    int64_t src_stride;
    const void* ref;
    int64_t ref_stride;
    int32_t height, width;
    const double* norm_in = nullptr;
    float* params_out = nullptr;
    int32_t n_param_bands = 0;
    void* corr_out = nullptr;
    double* norm_out = nullptr;
    uint64_t* r2_fail_count = nullptr;
    bool norm_only = false;  // hk_block_norm: the block statistics alone
    const hk_out_window* window = nullptr;
    uint8_t* valid_out = nullptr;  // nullable: the validity of the corrected window, rows window->stride bytes apart (packed without one)
};

// The whole host-pointer path: stage in (+ typed -> float32), (norm), fused kernel, (float32 -> typed) stage out.
// `io` nullable (float32 everywhere).
int run_host(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const HostFit& c) {
    const int32_t height = c.height, width = c.width;
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    int rc = validate_desc(desc);
    if (rc) return rc;
    if (!c.src || !c.ref) return fail(HK_ERR_ARG, "src/ref is NULL");
    if (height < 1 || width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d", height, width);
    if ((rc = check_strides(c.src_stride, width, c.ref_stride, width))) return rc;
    FitIo f;
    if ((rc = check_fit_io(desc, io, c.params_out, c.n_param_bands, &f, c.corr_out, c.valid_out))) return rc;
    if (!c.norm_only && !c.params_out && !c.corr_out) return fail(HK_ERR_ARG, "nothing to compute: params_out and corr_out are NULL");
    // output window (defaults: the whole block, written packed); param_stride is resolved to the row stride of params_out
    hk_out_window win = c.window ? *c.window : whole_block(height, width);
    if (c.window) {
        if (win.param_stride <= 0) win.param_stride = win.stride;
        if (win.row0 < 0 || win.col0 < 0 || win.rows < 1 || win.cols < 1 || win.row0 + win.rows > height || win.col0 + win.cols > width)
            return fail(HK_ERR_ARG, "output window outside the block");
        if ((c.corr_out && win.stride < win.cols) || (c.params_out && win.param_stride < win.cols))
            return fail(HK_ERR_ARG, "output row stride smaller than the window");
        if (c.params_out && c.n_param_bands > 1 && win.band_stride < (int64_t)(win.rows - 1) * win.param_stride + win.cols)
            return fail(HK_ERR_ARG, "output band stride smaller than a plane of the window");
    }
    HK_ENTER(ctx);

    const int64_t stride = row_align(width);
    const size_t plane = (size_t)stride * height * sizeof(float);
    const bool blk = desc->model == HK_MODEL_GAIN_BLK_OFFSET;
    const bool want_norm = blk || c.norm_only;
    const bool want_par = !c.norm_only && c.params_out, want_corr = !c.norm_only && c.corr_out;

    SlabLayout L;
    const size_t o_src = L.take(plane), o_ref = L.take(plane);
    const size_t o_gain = want_par ? L.take(plane) : 0, o_off = want_par ? L.take(plane) : 0;
    const size_t o_r2 = (want_par && c.n_param_bands == 3) ? L.take(plane) : 0;
    const size_t o_corr = want_corr ? L.take(plane) : 0;
    const size_t o_raw_o = (want_corr && f.out_cast) ? L.take((size_t)stride * height * hk::dtype_size(f.odt)) : 0;
    const size_t o_valid = (want_corr && f.want_valid) ? L.take((size_t)stride * height) : 0;
    const size_t o_raw_s = f.sdt ? L.take((size_t)stride * height * hk::dtype_size(f.sdt)) : 0;
    const size_t o_raw_r = f.rdt ? L.take((size_t)stride * height * hk::dtype_size(f.rdt)) : 0;
    const size_t o_aux = L.take(256);
    const size_t o_ws = want_norm ? L.take(hk::norm_workspace_bytes(1, height, width)) : 0;

    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    float *d_src = hc.at<float>(o_src), *d_ref = hc.at<float>(o_ref);
    float *d_gain = want_par ? hc.at<float>(o_gain) : nullptr, *d_off = want_par ? hc.at<float>(o_off) : nullptr;
    float* d_r2 = (want_par && c.n_param_bands == 3) ? hc.at<float>(o_r2) : nullptr;
    float* d_corr = want_corr ? hc.at<float>(o_corr) : nullptr;
    double* d_norm = hc.at<double>(o_aux);  // 2 doubles
    unsigned long long* d_fail = hc.at<unsigned long long>(o_aux + 64);
    void* d_ws = hc.at(o_ws);

    if ((rc = stage_in(sl, {c.src, c.src_stride, height, width}, f.sdt, d_src, hc.at(o_raw_s), stride))) return rc;
    if ((rc = stage_in(sl, {c.ref, c.ref_stride, height, width}, f.rdt, d_ref, hc.at(o_raw_r), stride))) return rc;
    if (c.norm_only) {
        HK_HIP(hk::launch_block_norm(norm_args(desc, d_src, d_ref, height, width, stride), d_ws, d_norm, sl.stream));
        HK_HIP(hipMemcpyAsync(sl.pin<double>(Slot::PIN_NORM), d_norm, 2 * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
        if ((rc = stage_finish(sl))) return rc;
        if (c.norm_out) memcpy(c.norm_out, sl.pin<double>(Slot::PIN_NORM), 2 * sizeof(double));
        return HK_OK;
    }

    // stage out: the window of the block the caller wants, straight into its (strided) arrays; the parameter planes lie one
    // plane apart in the slab
    const FitResults res = {.params_out = c.params_out, .n_param_bands = c.n_param_bands, .d_par = d_gain, .d_par_stride = stride,
                            .d_par_band = (int64_t)(o_off - o_gain) / 4, .pw = win, .corr_out = c.corr_out, .d_corr = d_corr,
                            .d_raw = hc.at(o_raw_o), .d_stride = stride, .height = height, .width = width, .cw = win,
                            .valid_out = c.valid_out, .d_valid = hc.at<unsigned char>(o_valid)};

    // The fit, its outputs and its r2-mask counter are queued back to back and the stream is synchronised ONCE; only
    // when pixels failed the mask do the in-painting passes follow, and the outputs are copied again behind them.
    FitPending pending;
    hk_dev_job job = {.src = d_src, .ref = d_ref, .gain = d_gain, .offset = d_off, .r2 = d_r2, .corr = d_corr, .norm = d_norm,
                      .fail_count = reinterpret_cast<uint64_t*>(d_fail), .n_bands = 1, .height = height, .width = width, .stride = stride};
    if (c.window && !f.out_cast) {  // the kernel's store window: the rows exactly, the columns from the window's first quad to the last column
        job.out_row0 = win.row0, job.out_rows = win.rows;
        job.out_col0 = win.col0 / hk::PX * hk::PX, job.out_cols = width - job.out_col0;
    }
    rc = fit_on_device(ctx, sl, desc, job, d_ws, c.norm_in, &pending);
    if (rc) return rc;
    if (c.norm_out && blk)
        HK_HIP(hipMemcpyAsync(sl.pin<double>(Slot::PIN_NORM), d_norm, 2 * sizeof(double), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = stage_fit_results(sl, f, res, /*d_fail=*/nullptr))) return rc;
    // hk_debug_fail_after_d2h(1) (homonim_hk_devtools.h): the call fails HERE, its result copies queued and not yet unpacked --
    // the state every HIP error between a stage_d2h and stage_finish leaves (tests/test_gpu_staging.py)
    if (g_fail_after_d2h.load(std::memory_order_relaxed))
        return fail(HK_ERR_HIP, "hk_debug_fail_after_d2h: injected failure behind the result copies");
    *sl.fail_host = 0;
    if (pending.active) HK_HIP(hipMemcpyAsync(sl.fail_host, d_fail, sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.stream));
    if ((rc = stage_finish(sl))) return rc;
    if (c.norm_out && blk) memcpy(c.norm_out, sl.pin<double>(Slot::PIN_NORM), 2 * sizeof(double));
    unsigned long long n_fail = *sl.fail_host;
    if (pending.active) {
        bool requeued = false;
        rc = fit_finish(ctx, sl, desc, pending, n_fail, &requeued);
        if (rc) return rc;
        if (requeued) {
            if ((rc = stage_fit_results(sl, f, res, d_fail))) return rc;
            if ((rc = stage_finish(sl))) return rc;
            n_fail = *sl.fail_host;  // (the in-painting passes do not count)
        }
    }
    if (c.r2_fail_count) *c.r2_fail_count = n_fail;
    return HK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Source and reference on DIFFERENT grids: the RefSpace and the SrcSpace chain.  Each chain of launches is stated once, for one
// band whose blocks are on the device; the host-pointer entries stage their blocks into the slab, run it and stage the results
// out, the device-resident entries run it band by band on the caller's planes and place the windows by device copies.

// One plane of a raster on the device: rows `stride` elements of its dtype apart.  staged: the host form put it where the chain's
// slab expects a staged block (a float32 plane in its place, another dtype in the raw plane, on the slab's stride)
struct DevGrid {
    const void* data;
    int64_t stride;
    int32_t height, width;
    bool staged = false;
};

// The plane `g` of dtype `dt` as the float32 plane `dplane` (row stride `dstride`) that the chains read.  A staged float32 plane
// lies there already; float32 elsewhere is copied.  Another dtype is converted by cast_in, which reads whole quads of a row: a
// staged plane (rows padded in the slab) and a caller's plane whose width is a multiple of the quad are read where they lie, any
// other goes through a copy in `raw` (the slab's stride, in elements of the dtype) -- a caller owns `width` elements of its last row
// and no more.
int bring_in(Slot& s, const DevGrid& g, int dt, float* dplane, void* raw, int64_t dstride) {
    const size_t es = hk::dtype_size(dt);
    const void* from = g.data;
    int64_t from_stride = g.stride;
    if (!dt) {
        if (!g.staged)
            HK_HIP(hipMemcpy2DAsync(dplane, dstride * es, from, from_stride * es, (size_t)g.width * es, g.height, hipMemcpyDeviceToDevice, s.stream));
        return HK_OK;
    }
    if (!g.staged && g.width % hk::PX != 0) {
        HK_HIP(hipMemcpy2DAsync(raw, dstride * es, from, from_stride * es, (size_t)g.width * es, g.height, hipMemcpyDeviceToDevice, s.stream));
        from = raw, from_stride = dstride;
    }
    HK_HIP(hk::launch_cast_in(dt, {.in = from, .in_stride = from_stride, .out = dplane, .out_stride = dstride, .height = g.height,
                                   .width = g.width}, s.stream));
    return HK_OK;
}

// ... and a host block staged to where `d` says (the slab)
int stage_grid(Slot& s, const HostGrid& g, int dt, const DevGrid& d) {
    const size_t es = hk::dtype_size(dt);
    return stage_h2d(s, const_cast<void*>(d.data), d.stride * es, g.data, g.stride * es, (size_t)g.width * es, g.height);
}

int check_refspace(const hk_space_desc* space) {
    for (int m : {space->down_resampling, space->up_resampling})
        if (!resampling_built(m)) return fail(HK_ERR_UNSUPPORTED, "resampling %d is not built", m);
    if (!(space->down[0] > 0 && space->down[2] > 0 && space->up[0] > 0 && space->up[2] > 0))
        return fail(HK_ERR_UNSUPPORTED, "flipped or degenerate grid mapping");
    return HK_OK;
}
int check_srcspace(const hk_srcspace_desc* space) {
    if (!resampling_built(space->resampling)) return fail(HK_ERR_UNSUPPORTED, "resampling %d is not built", space->resampling);
    if (!(space->map[0] > 0 && space->map[2] > 0)) return fail(HK_ERR_UNSUPPORTED, "flipped or degenerate grid mapping");
    return HK_OK;
}

// Where a chain left one band's results in its slab (FitResults' device side), and the band's r2-mask failure counter
struct ChainOut {
    const float* d_par;  // the parameter planes, d_par_band elements apart, rows d_par_stride apart
    int64_t d_par_stride, d_par_band;
    float* d_corr;       // the corrected plane, rows d_stride apart; d_raw / d_valid: where the cast writes
    void* d_raw;
    unsigned char* d_valid;
    int64_t d_stride;
    unsigned long long* d_fail;
};

// The slab of the RefSpace chain for one band: planes on the source grid (row stride ss) and on the reference grid (rs)
struct RefSpaceSlab {
    int64_t ss, rs;
    bool fused_up;  // bilinear / cubic_spline parameters are up-sampled inside the apply kernel (no full-resolution parameter planes)
    size_t o_src, o_ref, o_ds, o_gain, o_off, o_r2, o_gus, o_ous, o_corr, o_rowtab, o_vs, o_cov, o_mk, o_mkf, o_keep, o_cnt;
    size_t o_raw_s, o_raw_r, o_raw_o, o_valid, o_aux, o_ws, total;
};
RefSpaceSlab refspace_slab(const hk_fit_desc* desc, const FitIo& f, const hk_space_desc* space, int32_t sh, int32_t sw, int32_t rh,
                           int32_t rw) {
    RefSpaceSlab s;
    const int64_t ss = s.ss = row_align(sw), rs = s.rs = row_align(rw);
    const size_t splane = (size_t)ss * sh * 4, rplane = (size_t)rs * rh * 4;
    SlabLayout L;
    s.o_src = L.take(splane), s.o_ref = L.take(rplane), s.o_ds = L.take(rplane);
    s.o_gain = L.take(rplane), s.o_off = L.take(rplane), s.o_r2 = f.r2 ? L.take(rplane) : 0;
    s.fused_up = (space->up_resampling == 1 || space->up_resampling == 3) && rw >= 4 && space->up[0] <= 1.0 + 1e-9 &&
                 space->up[2] <= 1.0 + 1e-9 && (long long)rh * rs < 0x7fffffffLL;
    const bool fused_up = s.fused_up, partial = space->mask_partial != 0;
    s.o_gus = fused_up ? 0 : L.take(splane), s.o_ous = fused_up ? 0 : L.take(splane), s.o_corr = L.take(splane);
    s.o_rowtab = fused_up ? L.take(hk::upsample_apply_workspace_bytes(sh)) : 0;
    s.o_vs = partial ? L.take(splane) : 0, s.o_cov = partial ? L.take(rplane) : 0;
    s.o_mk = partial ? L.take((size_t)rs * rh) : 0;
    s.o_mkf = partial ? L.take(rplane) : 0, s.o_keep = partial ? L.take(splane) : 0;
    s.o_cnt = partial ? L.take((size_t)rs * rh * 2) : 0;
    s.o_raw_s = f.sdt ? L.take((size_t)ss * sh * hk::dtype_size(f.sdt)) : 0;
    s.o_raw_r = f.rdt ? L.take((size_t)rs * rh * hk::dtype_size(f.rdt)) : 0;
    s.o_raw_o = f.out_cast ? L.take((size_t)ss * sh * hk::dtype_size(f.odt)) : 0;
    s.o_valid = f.want_valid ? L.take((size_t)ss * sh) : 0;
    s.o_aux = L.take(256);
    s.o_ws = desc->model == HK_MODEL_GAIN_BLK_OFFSET ? L.take(hk::norm_workspace_bytes(1, rh, rw)) : 0;
    s.total = L.total;
    return s;
}

// RefSpaceModel.fit + RefSpaceModel.apply (homonim/kernel_model.py:476-503) of one band: sg / rg are its source and reference
// block on the device (dtypes f.sdt / f.rdt), `base` the slab L describes.  Queues on the slot's stream and waits only where
// fit_on_device does (gain-offset with an r2 threshold: once, for the failure count).
int refspace_chain(hk_ctx* ctx, Slot& sl, const hk_fit_desc* desc, const FitIo& f, const hk_space_desc* space, const RefSpaceSlab& L,
                   char* base, const DevGrid& sg, const DevGrid& rg, ChainOut* out) {
    int rc;
    const int64_t ss = L.ss, rs = L.rs;
    const int32_t src_height = sg.height, src_width = sg.width, ref_height = rg.height, ref_width = rg.width;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    float *d_src = F(L.o_src), *d_ref = F(L.o_ref), *d_ds = F(L.o_ds), *d_gain = F(L.o_gain), *d_off = F(L.o_off);
    float *d_r2 = f.r2 ? F(L.o_r2) : nullptr, *d_gus = F(L.o_gus), *d_ous = F(L.o_ous), *d_corr = F(L.o_corr);
    const int64_t par_band = (int64_t)(L.o_off - L.o_gain) / 4;  // gain -> offset plane, elements
    double* d_norm = reinterpret_cast<double*>(base + L.o_aux);
    unsigned long long* d_fail = reinterpret_cast<unsigned long long*>(base + L.o_aux + 64);
    const float nan = std::nanf("");

    if ((rc = bring_in(sl, sg, f.sdt, d_src, base + L.o_raw_s, ss))) return rc;
    if ((rc = bring_in(sl, rg, f.rdt, d_ref, base + L.o_raw_r, rs))) return rc;

    // one plane from the source grid down to the reference grid, or from there up to the source grid
    auto resample = [&](int mode, bool down, const float* from, int nd_mode, float nodata, float* to, float fill) {
        const DevGrid &a = down ? sg : rg, &b = down ? rg : sg;  // from a's shape to b's, on the slab's strides
        const hk::ResamplePlanes p = {.src = from, .dst = to, .src_stride = down ? ss : rs, .src_band_stride = 0, .dst_stride = down ? rs : ss,
                                      .dst_band_stride = 0, .sh = a.height, .sw = a.width, .dh = b.height, .dw = b.width, .n_bands = 1,
                                      .nd_mode = nd_mode, .nodata = nodata, .dst_fill = fill};
        const double* m = down ? space->down : space->up;
        return hk::launch_resample(mode, p, m[0], m[1], m[2], m[3], sl.stream);
    };

    // RefSpaceModel.fit (:476-482): source -> reference grid (nodata nan), then the base-class fit there
    HK_HIP(resample(space->down_resampling, true, d_src, desc->src_nodata_mode, desc->src_nodata, d_ds, nan));
    hk_fit_desc fd = *desc;
    fd.src_nodata_mode = HK_NODATA_NAN, fd.src_nodata = nan;
    const hk_dev_job job = {.src = d_ds, .ref = d_ref, .gain = d_gain, .offset = d_off, .r2 = d_r2, .norm = d_norm,
                            .fail_count = reinterpret_cast<uint64_t*>(d_fail), .n_bands = 1, .height = ref_height, .width = ref_width,
                            .stride = rs};
    if ((rc = fit_on_device(ctx, sl, &fd, job, base + L.o_ws))) return rc;

    // RefSpaceModel.apply (:484-503): gain / offset -> source grid, re-mask, apply
    if (!L.fused_up)
        for (int b = 0; b < 2; ++b)
            HK_HIP(resample(space->up_resampling, false, b ? d_off : d_gain, HK_NODATA_NAN, nan, b ? d_ous : d_gus, nan));
    const float* d_keep = nullptr;
    if (space->mask_partial) {
        // _full_coverage_mask (:375-409): source mask --average--> reference grid (>= 1) & parameter mask, eroded by
        // (kh+2) x (kw+2); back to the source grid with `nearest` (nodata 0)
        HK_HIP(hk::launch_valid_plane({.in = d_src, .in_stride = ss, .nd_mode = desc->src_nodata_mode, .nodata = desc->src_nodata,
                                       .out = F(L.o_vs), .out_stride = ss, .height = src_height, .width = src_width}, sl.stream));
        HK_HIP(resample(hk::RS_AVERAGE, true, F(L.o_vs), HK_NODATA_NONE, 0.f, F(L.o_cov), 0.f));
        unsigned char* d_mk = reinterpret_cast<unsigned char*>(base + L.o_mk);
        // the parameters as two bands: gain, and offset one band stride further on
        HK_HIP(hk::launch_partial_mask({.in = F(L.o_cov), .nd_mode = hk::ND_COVERAGE, .params = d_gain, .n_bands = 2, .band_stride = par_band,
                                        .height = ref_height, .width = ref_width, .stride = rs, .kh = desc->kh, .kw = desc->kw, .mask_out = d_mk},
                                       reinterpret_cast<unsigned short*>(base + L.o_cnt), sl.stream));
        HK_HIP(hk::launch_cast_in(HK_DTYPE_U8, {.in = d_mk, .in_stride = rs, .out = F(L.o_mkf), .out_stride = rs, .height = ref_height,
                                                .width = ref_width}, sl.stream));
        HK_HIP(resample(hk::RS_NEAREST, false, F(L.o_mkf), HK_NODATA_NONE, 0.f, F(L.o_keep), 0.f));
        d_keep = F(L.o_keep);
    }
    if (L.fused_up) {
        const double* up = space->up;
        HK_HIP(hk::launch_upsample_apply(space->up_resampling, {.src = d_src, .src_stride = ss, .nd_mode = desc->src_nodata_mode,
                                         .nodata = desc->src_nodata, .gain = d_gain, .offset = d_off, .par_stride = rs, .ph = ref_height,
                                         .pw = ref_width, .keep = d_keep, .keep_stride = ss, .out = d_corr, .out_stride = ss,
                                         .height = src_height, .width = src_width, .kx = up[0], .ox = up[1], .ky = up[2], .oy = up[3]},
                                         base + L.o_rowtab, sl.stream));
    } else {
        HK_HIP(hk::launch_apply_space({.src = d_src, .src_stride = ss, .nd_mode = desc->src_nodata_mode, .nodata = desc->src_nodata,
                                       .gain = d_gus, .offset = d_ous, .par_stride = ss, .keep = d_keep, .out = d_corr, .out_stride = ss,
                                       .height = src_height, .width = src_width}, sl.stream));
    }
    // the parameters on the reference grid, the corrected block on the source grid
    *out = {.d_par = d_gain, .d_par_stride = rs, .d_par_band = par_band, .d_corr = d_corr, .d_raw = base + L.o_raw_o,
            .d_valid = reinterpret_cast<unsigned char*>(base + L.o_valid), .d_stride = ss, .d_fail = d_fail};
    return HK_OK;
}

// The slab of the SrcSpace chain for one band; want_params: the (masked) parameter planes are an output
struct SrcSpaceSlab {
    int64_t ss, rs, pbs;  // pbs: band stride of the parameter planes, elements
    int n_par;
    bool typed_foot;      // `average` reads the reference as it lies there (footprint_typed_kernel): no float32 copy, no valid plane
    size_t o_src, o_rus, o_par, o_corr, o_cov, o_cnt, o_mpar, o_ref, o_vr, o_raw_s, o_raw_r, o_raw_o, o_valid, o_aux, o_ws, total;
};
SrcSpaceSlab srcspace_slab(const hk_fit_desc* desc, const FitIo& f, const hk_srcspace_desc* space, bool want_params, int32_t sh,
                           int32_t sw, int32_t rh, int32_t rw) {
    SrcSpaceSlab s;
    const int64_t ss = s.ss = row_align(sw), rs = s.rs = row_align(rw);
    const size_t splane = (size_t)ss * sh * 4, rplane = (size_t)rs * rh * 4;
    const bool partial = space->mask_partial != 0;
    const int n_par = s.n_par = f.r2 ? 3 : 2;
    const bool typed_foot = s.typed_foot = space->resampling == hk::RS_AVERAGE;
    SlabLayout L;
    s.o_src = L.take(splane), s.o_rus = L.take(splane);
    s.o_par = L.take(splane);  // gain, offset, (r2): planes of one size, one band stride apart
    for (int b = 1; b < n_par; ++b) L.take(splane);
    s.o_corr = L.take(splane);
    s.o_cov = partial ? L.take(splane) : 0, s.o_cnt = partial ? L.take((size_t)ss * sh * 2) : 0;
    s.o_mpar = (partial && want_params) ? L.take(splane) : 0;  // the masked parameters
    if (partial && want_params)
        for (int b = 1; b < n_par; ++b) L.take(splane);
    s.o_ref = (!typed_foot || !f.rdt) ? L.take(rplane) : 0, s.o_vr = (partial && !typed_foot) ? L.take(rplane) : 0;
    s.o_raw_s = f.sdt ? L.take((size_t)ss * sh * hk::dtype_size(f.sdt)) : 0;
    s.o_raw_r = f.rdt ? L.take((size_t)rs * rh * hk::dtype_size(f.rdt)) : 0;
    s.o_raw_o = f.out_cast ? L.take((size_t)ss * sh * hk::dtype_size(f.odt)) : 0;
    s.o_valid = f.want_valid ? L.take((size_t)ss * sh) : 0;
    s.o_aux = L.take(256);
    s.o_ws = desc->model == HK_MODEL_GAIN_BLK_OFFSET ? L.take(hk::norm_workspace_bytes(1, sh, sw)) : 0;
    s.pbs = (int64_t)((splane + 255) / 256 * 256 / 4);
    s.total = L.total;
    return s;
}

// SrcSpaceModel.fit + KernelModel.apply (homonim/kernel_model.py:506-535, :442-463) of one band, as refspace_chain states its own.
// With `average` the reference is read where rg says it lies, on rg's stride.
int srcspace_chain(hk_ctx* ctx, Slot& sl, const hk_fit_desc* desc, const FitIo& f, const hk_srcspace_desc* space, bool want_params,
                   const SrcSpaceSlab& L, char* base, const DevGrid& sg, const DevGrid& rg, ChainOut* out) {
    int rc;
    const int64_t ss = L.ss, rs = L.rs, pbs = L.pbs;
    const int32_t src_height = sg.height, src_width = sg.width, ref_height = rg.height, ref_width = rg.width;
    const bool r2 = f.r2, partial = space->mask_partial != 0;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    float *d_src = F(L.o_src), *d_rus = F(L.o_rus), *d_gain = F(L.o_par), *d_off = d_gain + pbs, *d_r2 = r2 ? d_gain + 2 * pbs : nullptr;
    float* d_corr = F(L.o_corr);
    double* d_norm = reinterpret_cast<double*>(base + L.o_aux);
    unsigned long long* d_fail = reinterpret_cast<unsigned long long*>(base + L.o_aux + 64);
    const float nan = std::nanf("");
    const double* m = space->map;

    if ((rc = bring_in(sl, sg, f.sdt, d_src, base + L.o_raw_s, ss))) return rc;

    // SrcSpaceModel.fit (:520): reference -> source grid (nodata nan), and for mask_partial the coverage of its valid mask
    // (_full_coverage_mask, :375-399: mask_ra re-projected with `average`, no nodata)
    if (L.typed_foot) {
        HK_HIP(hk::launch_footprint_typed(f.rdt, {.src = rg.data, .src_stride = rg.stride, .sh = ref_height, .sw = ref_width,
                                                  .nd_mode = desc->ref_nodata_mode, .nodata = desc->ref_nodata, .value = d_rus,
                                                  .coverage = partial ? F(L.o_cov) : nullptr, .dst_stride = ss, .dh = src_height,
                                                  .dw = src_width, .fill = nan, .kx = m[0], .ox = m[1], .ky = m[2], .oy = m[3]},
                                          sl.stream));
    } else {
        float* d_ref = F(L.o_ref);
        if ((rc = bring_in(sl, rg, f.rdt, d_ref, base + L.o_raw_r, rs))) return rc;
        hk::ResamplePlanes p = {.src = d_ref, .dst = d_rus, .src_stride = rs, .src_band_stride = 0, .dst_stride = ss, .dst_band_stride = 0,
                                .sh = rg.height, .sw = rg.width, .dh = sg.height, .dw = sg.width, .n_bands = 1,
                                .nd_mode = desc->ref_nodata_mode, .nodata = desc->ref_nodata, .dst_fill = nan};
        HK_HIP(hk::launch_resample(space->resampling, p, m[0], m[1], m[2], m[3], sl.stream));
        if (partial) {
            HK_HIP(hk::launch_valid_plane({.in = d_ref, .in_stride = rs, .nd_mode = desc->ref_nodata_mode, .nodata = desc->ref_nodata,
                                           .out = F(L.o_vr), .out_stride = rs, .height = ref_height, .width = ref_width}, sl.stream));
            p.src = F(L.o_vr), p.dst = F(L.o_cov), p.nd_mode = HK_NODATA_NONE, p.nodata = 0.f, p.dst_fill = 0.f;
            HK_HIP(hk::launch_resample(hk::RS_AVERAGE, p, m[0], m[1], m[2], m[3], sl.stream));
        }
    }

    // KernelModel.fit on the source grid; without mask_partial the fused kernel applies as well: the parameters are nodata
    // wherever the source is, so that masking them with the source mask (:533) changes nothing
    hk_fit_desc fd = *desc;
    fd.ref_nodata_mode = HK_NODATA_NAN, fd.ref_nodata = nan;
    const hk_dev_job job = {.src = d_src, .ref = d_rus, .gain = d_gain, .offset = d_off, .r2 = d_r2, .corr = partial ? nullptr : d_corr,
                            .norm = d_norm, .fail_count = reinterpret_cast<uint64_t*>(d_fail), .n_bands = 1, .height = src_height,
                            .width = src_width, .stride = ss};
    if ((rc = fit_on_device(ctx, sl, &fd, job, base + L.o_ws))) return rc;

    float* d_pout = d_gain;
    if (partial) {
        // :526-531: coverage >= 1 & "has gain or offset", eroded by (kh+2) x (kw+2), on ALL parameter bands; then KernelModel.apply
        d_pout = want_params ? F(L.o_mpar) : nullptr;
        HK_HIP(hk::launch_partial_mask({.in = F(L.o_cov), .nd_mode = hk::ND_COVERAGE, .params = d_gain, .n_bands = L.n_par, .band_stride = pbs,
                                        .src = d_src, .height = src_height, .width = src_width, .stride = ss, .kh = desc->kh,
                                        .kw = desc->kw, .params_out = d_pout, .corr_out = d_corr},
                                       reinterpret_cast<unsigned short*>(base + L.o_cnt), sl.stream));
    }
    *out = {.d_par = d_pout, .d_par_stride = ss, .d_par_band = pbs, .d_corr = d_corr, .d_raw = base + L.o_raw_o,
            .d_valid = reinterpret_cast<unsigned char*>(base + L.o_valid), .d_stride = ss, .d_fail = d_fail};
    return HK_OK;
}

// The two store windows of a device-resident two-grid job as place_fit_results takes them (FitResults::cw, ::pw): all zero in
// the job = the whole grid.  Resolved here, once.
struct TwoGridWindows {
    hk_out_window cw, pw;
};

// What a device-resident two-grid job asks beyond what the host forms check: n_bands, the reserved word, windows (resolved into
// *w), strides, planes that overlap, and -- with a context -- the stream and the caller's scratch (`need` bytes).  `ph` x `pw`: the
// parameter grid.  ctx NULL: the scratch-size helpers, which have no stream pool and do not look at the job's own scratch.
int check_two_grid_job(const hk_ctx* ctx, const hk_two_grid_job* j, int32_t ph, int32_t pw, uint64_t need, TwoGridWindows* w) {
    if (j->n_bands < 1) return fail(HK_ERR_ARG, "n_bands must be at least 1");
    if (j->reserved != 0) return fail(HK_ERR_ARG, "hk_two_grid_job.reserved must be 0");
    // -> 0: the window inside a grid of rows x cols (all zero: the whole grid), 1: outside it
    auto resolve = [](int32_t row0, int32_t col0, int32_t nrows, int32_t ncols, int32_t rows, int32_t cols, hk_out_window* out) {
        if (!(row0 || col0 || nrows || ncols)) nrows = rows, ncols = cols;
        if (row0 < 0 || col0 < 0 || nrows < 1 || ncols < 1 || row0 + (int64_t)nrows > rows || col0 + (int64_t)ncols > cols) return 1;
        out->row0 = row0, out->col0 = col0, out->rows = nrows, out->cols = ncols;
        return 0;
    };
    if (resolve(j->out_row0, j->out_col0, j->out_rows, j->out_cols, j->src_height, j->src_width, &w->cw))
        return fail(HK_ERR_ARG, "output window outside the block");
    if (resolve(j->par_row0, j->par_col0, j->par_rows, j->par_cols, ph, pw, &w->pw))
        return fail(HK_ERR_ARG, "parameter window outside the parameter grid");
    w->cw.stride = j->corr_stride, w->cw.band_stride = 0, w->cw.param_stride = 0;
    w->pw.stride = w->pw.param_stride = j->param_stride, w->pw.band_stride = (int64_t)j->n_bands * j->param_band_stride;
    const hk_out_window &cw = w->cw, &pwin = w->pw;
    if (j->corr_stride < cw.cols || (j->valid && j->valid_stride < cw.cols) || (j->params && j->param_stride < pwin.cols))
        return fail(HK_ERR_ARG, "output row stride smaller than the window");
    // planes of one array must not overlap: a band stride spans at least the rows that are read or written
    auto spans = [](int64_t band_stride, int64_t stride, int64_t rows, int64_t cols) { return band_stride >= (rows - 1) * stride + cols; };
    if (j->n_bands > 1 && (!spans(j->src_band_stride, j->src_stride, j->src_height, j->src_width) ||
                           !spans(j->ref_band_stride, j->ref_stride, j->ref_height, j->ref_width) ||
                           !spans(j->corr_band_stride, j->corr_stride, cw.rows, cw.cols) ||
                           (j->valid && !spans(j->valid_band_stride, j->valid_stride, cw.rows, cw.cols))))
        return fail(HK_ERR_ARG, "band stride smaller than a plane: the planes overlap");
    if (j->params && !spans(j->param_band_stride, j->param_stride, pwin.rows, pwin.cols))
        return fail(HK_ERR_ARG, "band stride smaller than a plane: the planes overlap");
    if (!ctx) return HK_OK;
    if (const int rc = check_stream(ctx, j->stream)) return rc;
    if (j->scratch) {
        if ((uintptr_t)j->scratch & 255) return fail(HK_ERR_ARG, "job scratch must be 256-byte aligned");
        if (j->scratch_bytes < need)
            return fail(HK_ERR_ARG, "job scratch of %llu bytes is smaller than the %llu bytes this job needs", (unsigned long long)j->scratch_bytes,
                        (unsigned long long)need);
    }
    return HK_OK;
}

// Everything a device-resident two-grid call is refused for, in the host form's order and words where the check is shared; the
// slab of one band (*L) and the resolved windows (*w).  ctx NULL: the scratch-size helpers (check_two_grid_job).
template <class Space, class Slab>
int check_two_grid_dev(const hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const Space* space, const hk_two_grid_job* j,
                       FitIo* f, Slab* L, TwoGridWindows* w) {
    if (!j) return null_arg();
    const DevGrid sg = {j->src, j->src_stride, j->src_height, j->src_width}, rg = {j->ref, j->ref_stride, j->ref_height, j->ref_width};
    int rc = check_two_grid_args(desc, space, sg, rg, j->corr);
    if (rc) return rc;
    if constexpr (std::is_same_v<Space, hk_space_desc>) rc = check_refspace(space);
    else rc = check_srcspace(space);
    if (rc || (rc = check_fit_io(desc, io, j->params, j->n_param_bands, f, j->corr, j->valid))) return rc;
    int32_t ph, pw;
    if constexpr (std::is_same_v<Space, hk_space_desc>) {
        *L = refspace_slab(desc, *f, space, j->src_height, j->src_width, j->ref_height, j->ref_width);
        ph = j->ref_height, pw = j->ref_width;
    } else {
        *L = srcspace_slab(desc, *f, space, j->params != nullptr, j->src_height, j->src_width, j->ref_height, j->ref_width);
        ph = j->src_height, pw = j->src_width;
    }
    return check_two_grid_job(ctx, j, ph, pw, L->total, w);
}

// One device-resident two-grid call: the refusals, the scratch, then `chain` band by band on the job's stream, each band's
// windows placed behind it.  The bands share one band's slab in stream order.
template <class Space, class Slab, class Chain>
int two_grid_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const Space* space, const hk_two_grid_job* j,
                 uint64_t* n_fail_out, Chain chain) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    FitIo f;
    Slab L;
    TwoGridWindows w;
    int rc = check_two_grid_dev(ctx, desc, io, space, j, &f, &L, &w);
    if (rc) return rc;
    DevEnter entered(ctx, j->stream);
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[j->stream];
    char* base = static_cast<char*>(j->scratch);
    if (!base) {
        std::lock_guard<std::mutex> lk(ctx->mu);  // (as ensure_stream_ws: the slab may be reallocated)
        if ((rc = ensure_dev(sl, L.total))) return rc;
        base = static_cast<char*>(sl.dev);
    }
    const bool counts = desc->model == HK_MODEL_GAIN_OFFSET && desc->has_r2_thresh;
    const size_t ses = hk::dtype_size(f.sdt), res = hk::dtype_size(f.rdt), oes = hk::dtype_size(f.odt);
    for (int64_t b = 0; b < j->n_bands; ++b) {
        const DevGrid sg = {static_cast<const char*>(j->src) + b * j->src_band_stride * (int64_t)ses, j->src_stride, j->src_height, j->src_width};
        const DevGrid rg = {static_cast<const char*>(j->ref) + b * j->ref_band_stride * (int64_t)res, j->ref_stride, j->ref_height, j->ref_width};
        ChainOut o;
        if ((rc = chain(sl, f, L, base, sg, rg, &o))) return rc;
        if (n_fail_out) n_fail_out[b] = counts ? *sl.fail_host : 0;  // (fit_on_device has waited for it)
        FitResults res_b = {.params_out = j->params ? j->params + b * j->param_band_stride : nullptr, .n_param_bands = j->n_param_bands,
                            .d_par = o.d_par, .d_par_stride = o.d_par_stride, .d_par_band = o.d_par_band, .pw = w.pw,
                            .corr_out = static_cast<char*>(j->corr) + b * j->corr_band_stride * (int64_t)oes, .d_corr = o.d_corr,
                            .d_raw = o.d_raw, .d_stride = o.d_stride, .height = j->src_height, .width = j->src_width, .cw = w.cw,
                            .valid_out = j->valid ? j->valid + b * j->valid_band_stride : nullptr, .d_valid = o.d_valid};
        if ((rc = place_fit_results(sl, f, res_b, j->valid_stride))) return rc;
    }
    return HK_OK;
}

}  // namespace

extern "C" {

int hk_abi_version(void) { return HK_ABI_VERSION; }
const char* hk_backend_name(void) { return "hip-gfx950"; }
const char* hk_last_error(void) { return g_err; }

int hk_device_count(int* count) {
    if (!count) return fail(HK_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(HK_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return HK_OK;
}

int hk_device_pci_bus_id(int device_id, char* out, int len) {
    if (!out || len < 13) return fail(HK_ERR_ARG, "bus-id buffer is NULL or shorter than 13 bytes");
    out[0] = '\0';
    hipError_t e = hipDeviceGetPCIBusId(out, len, device_id);
    if (e != hipSuccess) return fail(HK_ERR_NODEVICE, "hipDeviceGetPCIBusId(%d): %s", device_id, hipGetErrorString(e));
    for (char* c = out; *c; ++c) *c = (char)tolower((unsigned char)*c);   // sysfs spells bus addresses in lower case
    return HK_OK;
}

int hk_ctx_create(int device_id, int n_streams, hk_ctx** out) {
    if (!out) return fail(HK_ERR_ARG, "ctx out-pointer is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return fail(HK_ERR_NODEVICE, "no HIP device available (libhomonim_hk needs an MI355X / gfx950 GPU)");
    if (device_id < 0 || device_id >= n) return fail(HK_ERR_ARG, "device %d out of range [0, %d)", device_id, n);
    if (n_streams < 1) n_streams = 1;
    if (n_streams > 64) n_streams = 64;
    HK_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HK_HIP(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(HK_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
    hk_ctx* ctx = new (std::nothrow) hk_ctx();
    if (!ctx) return fail(HK_ERR_NOMEM, "out of host memory");
    ctx->device = device_id;
    ctx->slots.resize(n_streams);
    {
        auto env = [](const char* name) { const char* e = getenv(name); return e ? std::optional<int>(atoi(e)) : std::nullopt; };
        LaunchPolicy& lp = ctx->launch;
        if (const auto remap = env("HK_XCD_REMAP")) lp.xcd_remap = std::min(std::max(*remap, 0), 256);
        lp.force_general = env("HK_FORCE_GENERAL").value_or(0);
        lp.use_ring = env("HK_USE_RING");
        lp.wave_slots = env("HK_WAVE_SLOTS").value_or(lp.wave_slots);
        lp.seg_big = env("HK_SEG_BIG");
        lp.seg_tail = env("HK_SEG_TAIL");
    }
    for (auto& s : ctx->slots) {
        hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            hk_ctx_destroy(ctx);
            return fail(HK_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        if (ensure_pin(s) != HK_OK) {
            hk_ctx_destroy(ctx);
            return HK_ERR_NOMEM;
        }
    }
    {
        hipError_t e = hipStreamCreateWithFlags(&ctx->xfer.stream, hipStreamNonBlocking);
        if (e != hipSuccess || ensure_pin(ctx->xfer) != HK_OK) {
            hk_ctx_destroy(ctx);
            return e != hipSuccess ? fail(HK_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)) : HK_ERR_NOMEM;
        }
    }
    register_gpu_fault_report();  // (HIP, and with it the HSA runtime, is up: the streams above were created on it)
    *out = ctx;
    return HK_OK;
}

int hk_ctx_destroy(hk_ctx* ctx) {
    if (!ctx) return HK_OK;
    (void)hipSetDevice(ctx->device);
    for (auto& s : ctx->slots) slot_release(s);
    slot_release(ctx->xfer);
    if (ctx->comm && rccl().ok) rccl().CommDestroy(ctx->comm);
    delete ctx;
    return HK_OK;
}

int hk_ctx_sync(hk_ctx* ctx) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    HK_ENTER(ctx);
    HK_HIP(hipDeviceSynchronize());
    return HK_OK;
}

int hk_block_norm(hk_ctx* ctx, const hk_fit_desc* desc, const float* src, int64_t src_stride, const float* ref,
                  int64_t ref_stride, int32_t height, int32_t width, double norm_out[2]) {
    if (!norm_out) return fail(HK_ERR_ARG, "norm_out is NULL");
    return run_host(ctx, desc, nullptr, {.src = src, .src_stride = src_stride, .ref = ref, .ref_stride = ref_stride, .height = height,
                                         .width = width, .norm_out = norm_out, .norm_only = true});
}

int hk_fit(hk_ctx* ctx, const hk_fit_desc* desc, const float* src, int64_t src_stride, const float* ref,
           int64_t ref_stride, int32_t height, int32_t width, const double* norm_in, float* params_out,
           int32_t n_param_bands, double* norm_out, uint64_t* r2_fail_count) {
    if (!params_out) return fail(HK_ERR_ARG, "params_out is NULL");
    return run_host(ctx, desc, nullptr, {.src = src, .src_stride = src_stride, .ref = ref, .ref_stride = ref_stride, .height = height,
                                         .width = width, .norm_in = norm_in, .params_out = params_out, .n_param_bands = n_param_bands,
                                         .norm_out = norm_out, .r2_fail_count = r2_fail_count});
}

int hk_fit_apply(hk_ctx* ctx, const hk_fit_desc* desc, const float* src, int64_t src_stride, const float* ref,
                 int64_t ref_stride, int32_t height, int32_t width, const double* norm_in, float* params_out,
                 int32_t n_param_bands, float* corr_out, double* norm_out, uint64_t* r2_fail_count) {
    if (!corr_out) return fail(HK_ERR_ARG, "corr_out is NULL");
    return run_host(ctx, desc, nullptr, {.src = src, .src_stride = src_stride, .ref = ref, .ref_stride = ref_stride, .height = height,
                                         .width = width, .norm_in = norm_in, .params_out = params_out, .n_param_bands = n_param_bands,
                                         .corr_out = corr_out, .norm_out = norm_out, .r2_fail_count = r2_fail_count});
}

int hk_fit_apply_io(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const void* src, int64_t src_stride,
                    const void* ref, int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                    float* params_out, int32_t n_param_bands, void* corr_out, double* norm_out, uint64_t* r2_fail_count) {
    return run_host(ctx, desc, io, {.src = src, .src_stride = src_stride, .ref = ref, .ref_stride = ref_stride, .height = height,
                                    .width = width, .norm_in = norm_in, .params_out = params_out, .n_param_bands = n_param_bands,
                                    .corr_out = corr_out, .norm_out = norm_out, .r2_fail_count = r2_fail_count});
}

int hk_fit_apply_block_valid(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const void* src, int64_t src_stride,
                             const void* ref, int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                             float* params_out, int32_t n_param_bands, void* corr_out, uint8_t* valid_out,
                             const hk_out_window* window, double* norm_out, uint64_t* r2_fail_count) {
    return run_host(ctx, desc, io, {.src = src, .src_stride = src_stride, .ref = ref, .ref_stride = ref_stride, .height = height,
                                    .width = width, .norm_in = norm_in, .params_out = params_out, .n_param_bands = n_param_bands,
                                    .corr_out = corr_out, .norm_out = norm_out, .r2_fail_count = r2_fail_count, .window = window,
                                    .valid_out = valid_out});
}

int hk_fit_apply_block(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const void* src, int64_t src_stride,
                       const void* ref, int64_t ref_stride, int32_t height, int32_t width, const double* norm_in,
                       float* params_out, int32_t n_param_bands, void* corr_out, const hk_out_window* window,
                       double* norm_out, uint64_t* r2_fail_count) {
    return hk_fit_apply_block_valid(ctx, desc, io, src, src_stride, ref, ref_stride, height, width, norm_in, params_out,
                                    n_param_bands, corr_out, /*valid_out=*/nullptr, window, norm_out, r2_fail_count);
}

int hk_apply(hk_ctx* ctx, const float* src, int64_t src_stride, const float* params, int32_t height, int32_t width,
             float* out) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!src || !params || !out) return null_arg();
    if (height < 1 || width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d", height, width);
    int rc = check_strides(src_stride, width);
    if (rc) return rc;
    HK_ENTER(ctx);
    const int64_t stride = row_align(width);
    const size_t plane = (size_t)stride * height * sizeof(float);
    SlabLayout L;
    const size_t o_src = L.take(plane), o_gain = L.take(plane), o_off = L.take(plane), o_out = L.take(plane);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    float *d_src = hc.at<float>(o_src), *d_gain = hc.at<float>(o_gain), *d_off = hc.at<float>(o_off), *d_out = hc.at<float>(o_out);
    const size_t wbytes = (size_t)width * sizeof(float);
    if ((rc = stage_h2d(hc.sl, d_src, stride * 4, src, src_stride * 4, wbytes, height))) return rc;
    if ((rc = stage_h2d(hc.sl, d_gain, stride * 4, params, wbytes, wbytes, height))) return rc;
    if ((rc = stage_h2d(hc.sl, d_off, stride * 4, params + (size_t)height * width, wbytes, wbytes, height))) return rc;
    HK_HIP(hk::launch_apply(d_src, d_gain, d_off, d_out, height, width, stride, hc.sl.stream));
    if ((rc = stage_d2h(hc.sl, out, wbytes, d_out, stride * 4, wbytes, height))) return rc;
    return stage_finish(hc.sl);
}

int hk_refspace_fit_apply_valid(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                                const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                                int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                                int32_t n_param_bands, void* corr_out, uint8_t* valid_out, uint64_t* r2_fail_count) {
    const HostGrid sg = {src, src_stride, src_height, src_width}, rg = {ref, ref_stride, ref_height, ref_width};
    int rc = check_two_grids(ctx, desc, space, sg, rg, corr_out);
    if (rc || (rc = check_refspace(space))) return rc;
    FitIo f;
    if ((rc = check_fit_io(desc, io, params_out, n_param_bands, &f, corr_out, valid_out))) return rc;
    HK_ENTER(ctx);

    const RefSpaceSlab L = refspace_slab(desc, f, space, src_height, src_width, ref_height, ref_width);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    // stage in: each block where the chain's bring_in expects a staged one, on the slab's strides
    const DevGrid d_sg = {hc.at(f.sdt ? L.o_raw_s : L.o_src), L.ss, src_height, src_width, /*staged=*/true};
    const DevGrid d_rg = {hc.at(f.rdt ? L.o_raw_r : L.o_ref), L.rs, ref_height, ref_width, /*staged=*/true};
    if ((rc = stage_grid(sl, sg, f.sdt, d_sg)) || (rc = stage_grid(sl, rg, f.rdt, d_rg))) return rc;
    ChainOut o;
    if ((rc = refspace_chain(ctx, sl, desc, f, space, L, hc.at(0), d_sg, d_rg, &o))) return rc;

    // stage out: the parameters on the reference grid, the corrected block on the source grid, both whole and packed
    const FitResults res = {.params_out = params_out, .n_param_bands = n_param_bands, .d_par = o.d_par, .d_par_stride = o.d_par_stride,
                            .d_par_band = o.d_par_band, .pw = whole_block(ref_height, ref_width), .corr_out = corr_out, .d_corr = o.d_corr,
                            .d_raw = o.d_raw, .d_stride = o.d_stride, .height = src_height, .width = src_width,
                            .cw = whole_block(src_height, src_width), .valid_out = valid_out, .d_valid = o.d_valid};
    if ((rc = stage_fit_results(sl, f, res, o.d_fail))) return rc;
    if ((rc = stage_finish(sl))) return rc;
    if (r2_fail_count) *r2_fail_count = *sl.fail_host;
    return HK_OK;
}

int hk_refspace_fit_apply(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                          const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                          int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                          int32_t n_param_bands, void* corr_out, uint64_t* r2_fail_count) {
    return hk_refspace_fit_apply_valid(ctx, desc, io, space, src, src_stride, src_height, src_width, ref, ref_stride, ref_height,
                                       ref_width, params_out, n_param_bands, corr_out, /*valid_out=*/nullptr, r2_fail_count);
}

int hk_srcspace_fit_apply_valid(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                                const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                                int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                                int32_t n_param_bands, void* corr_out, uint8_t* valid_out, uint64_t* r2_fail_count) {
    const HostGrid sg = {src, src_stride, src_height, src_width}, rg = {ref, ref_stride, ref_height, ref_width};
    int rc = check_two_grids(ctx, desc, space, sg, rg, corr_out);
    if (rc || (rc = check_srcspace(space))) return rc;
    FitIo f;
    if ((rc = check_fit_io(desc, io, params_out, n_param_bands, &f, corr_out, valid_out))) return rc;
    HK_ENTER(ctx);

    const SrcSpaceSlab L = srcspace_slab(desc, f, space, params_out != nullptr, src_height, src_width, ref_height, ref_width);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    // stage in: each block where the chain expects a staged one, on the slab's strides (`average` reads the reference there as it is)
    const DevGrid d_sg = {hc.at(f.sdt ? L.o_raw_s : L.o_src), L.ss, src_height, src_width, /*staged=*/true};
    const DevGrid d_rg = {hc.at(f.rdt ? L.o_raw_r : L.o_ref), L.rs, ref_height, ref_width, /*staged=*/true};
    if ((rc = stage_grid(sl, sg, f.sdt, d_sg)) || (rc = stage_grid(sl, rg, f.rdt, d_rg))) return rc;
    ChainOut o;
    if ((rc = srcspace_chain(ctx, sl, desc, f, space, params_out != nullptr, L, hc.at(0), d_sg, d_rg, &o))) return rc;

    // stage out: the parameters and the corrected block on the source grid, whole and packed
    const hk_out_window whole = whole_block(src_height, src_width);
    const FitResults res = {.params_out = params_out, .n_param_bands = n_param_bands, .d_par = o.d_par, .d_par_stride = o.d_par_stride,
                            .d_par_band = o.d_par_band, .pw = whole, .corr_out = corr_out, .d_corr = o.d_corr, .d_raw = o.d_raw,
                            .d_stride = o.d_stride, .height = src_height, .width = src_width, .cw = whole, .valid_out = valid_out,
                            .d_valid = o.d_valid};
    if ((rc = stage_fit_results(sl, f, res, o.d_fail))) return rc;
    if ((rc = stage_finish(sl))) return rc;
    if (r2_fail_count) *r2_fail_count = *sl.fail_host;
    return HK_OK;
}

int hk_srcspace_fit_apply(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                          const void* src, int64_t src_stride, int32_t src_height, int32_t src_width, const void* ref,
                          int64_t ref_stride, int32_t ref_height, int32_t ref_width, float* params_out,
                          int32_t n_param_bands, void* corr_out, uint64_t* r2_fail_count) {
    return hk_srcspace_fit_apply_valid(ctx, desc, io, space, src, src_stride, src_height, src_width, ref, ref_stride, ref_height,
                                       ref_width, params_out, n_param_bands, corr_out, /*valid_out=*/nullptr, r2_fail_count);
}

uint64_t hk_refspace_dev_scratch_bytes(const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                                       const hk_two_grid_job* job) {
    FitIo f;
    RefSpaceSlab L;
    TwoGridWindows w;
    return check_two_grid_dev(nullptr, desc, io, space, job, &f, &L, &w) ? 0 : L.total;
}
uint64_t hk_srcspace_dev_scratch_bytes(const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                                       const hk_two_grid_job* job) {
    FitIo f;
    SrcSpaceSlab L;
    TwoGridWindows w;
    return check_two_grid_dev(nullptr, desc, io, space, job, &f, &L, &w) ? 0 : L.total;
}

int hk_refspace_fit_apply_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_space_desc* space,
                              const hk_two_grid_job* job, uint64_t* n_fail_out) {
    return two_grid_dev<hk_space_desc, RefSpaceSlab>(
        ctx, desc, io, space, job, n_fail_out,
        [&](Slot& sl, const FitIo& f, const RefSpaceSlab& L, char* base, const DevGrid& sg, const DevGrid& rg, ChainOut* o) {
            return refspace_chain(ctx, sl, desc, f, space, L, base, sg, rg, o);
        });
}

int hk_srcspace_fit_apply_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_io_desc* io, const hk_srcspace_desc* space,
                              const hk_two_grid_job* job, uint64_t* n_fail_out) {
    return two_grid_dev<hk_srcspace_desc, SrcSpaceSlab>(
        ctx, desc, io, space, job, n_fail_out,
        [&](Slot& sl, const FitIo& f, const SrcSpaceSlab& L, char* base, const DevGrid& sg, const DevGrid& rg, ChainOut* o) {
            return srcspace_chain(ctx, sl, desc, f, space, job->params != nullptr, L, base, sg, rg, o);
        });
}

int hk_reproject(hk_ctx* ctx, const float* src, int32_t n_bands, int32_t src_height, int32_t src_width,
                 int32_t src_nodata_mode, float src_nodata, double kx, double ox, double ky, double oy, int32_t resampling,
                 float* dst, int32_t dst_height, int32_t dst_width, float dst_fill) {
    const hk::ResamplePlanes p = {.src = src, .dst = dst, .sh = src_height, .sw = src_width, .dh = dst_height, .dw = dst_width,
                                  .n_bands = n_bands, .nd_mode = src_nodata_mode, .nodata = src_nodata, .dst_fill = dst_fill};
    const int rc = check_reproject(ctx, p, kx, ky, resampling, /*host_form=*/true);
    if (rc) return rc;
    return reproject_packed(ctx, p, [&](const hk::ResamplePlanes& slab, hipStream_t stream) {
        HK_HIP(hk::launch_resample(resampling, slab, kx, ox, ky, oy, stream));
        return (int)HK_OK;
    });
}

int hk_reproject_dev(hk_ctx* ctx, const float* src_dev, int32_t n_bands, int32_t src_height, int32_t src_width,
                     int64_t src_stride, int64_t src_band_stride, int32_t src_nodata_mode, float src_nodata, double kx, double ox,
                     double ky, double oy, int32_t resampling, float* dst_dev, int32_t dst_height, int32_t dst_width,
                     int64_t dst_stride, int64_t dst_band_stride, float dst_fill, int32_t stream) {
    const hk::ResamplePlanes p = {.src = src_dev, .dst = dst_dev, .src_stride = src_stride, .src_band_stride = src_band_stride,
                                  .dst_stride = dst_stride, .dst_band_stride = dst_band_stride, .sh = src_height, .sw = src_width,
                                  .dh = dst_height, .dw = dst_width, .n_bands = n_bands, .nd_mode = src_nodata_mode, .nodata = src_nodata,
                                  .dst_fill = dst_fill};
    int rc = check_reproject(ctx, p, kx, ky, resampling, /*host_form=*/false);
    if (rc) return rc;
    if ((rc = check_resample_strides(p)) || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    HK_HIP(hk::launch_resample(resampling, p, kx, ox, ky, oy, ctx->slots[stream].stream));
    return HK_OK;
}

// Re-sampling between grids of two CRSs and between rotated / sheared grids (hk_warp.hip): see include/homonim_hk.h.  The entry
// points of hk_warp_desc and of hk_affine_warp_desc share their bodies; hk::launch_warp_* is overloaded on the descriptor.
static int check_warp_lattice(hk_ctx* ctx, const void* warp, const hk::WarpLattice& l) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!warp || !l.x || !l.y) return null_arg();
    if (l.h < 1 || l.w < 1) return fail(HK_ERR_ARG, "empty lattice %d x %d", l.h, l.w);
    if (l.h > 65535) return fail(HK_ERR_UNSUPPORTED, "lattice taller than 65535 rows");
    return check_strides(l.stride, l.w);
}

// hipErrorInvalidValue of the warp launchers carries a reason: an unusable descriptor (HK_ERR_ARG), or CRSs the warp is not
// built for (different ellipsoids: HK_ERR_UNSUPPORTED)
static int warp_launch_status(hipError_t e, const char* why) {
    if (e == hipSuccess) return HK_OK;
    (void)hipGetLastError();
    if (e == hipErrorInvalidValue && why)
        return fail(strstr(why, "ellipsoids") ? HK_ERR_UNSUPPORTED : HK_ERR_ARG, "warp: %s", why);
    return fail(HK_ERR_HIP, "warp launch failed: %s", hipGetErrorString(e));
}

extern "C++" template <typename Desc>
static int warp_coords_dev(hk_ctx* ctx, const Desc* warp, const hk::WarpLattice& l, int32_t stream) {
    int rc = check_warp_lattice(ctx, warp, l);
    if (rc || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    const char* why = nullptr;
    return warp_launch_status(hk::launch_warp_coords(warp, l, ctx->slots[stream].stream, &why), why);
}

// (`out`: the caller's host planes; the lattice is computed into the slab at the device row stride and copied there)
extern "C++" template <typename Desc>
static int warp_coords_host(hk_ctx* ctx, const Desc* warp, const hk::WarpLattice& out) {
    int rc = check_warp_lattice(ctx, warp, out);
    if (rc) return rc;
    HK_ENTER(ctx);
    const int64_t d_stride = row_align(out.w);
    SlabLayout L;
    const size_t plane = (size_t)d_stride * out.h * sizeof(double);
    const size_t o_x = L.take(plane), o_y = L.take(plane);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    const char* why = nullptr;
    hk::WarpLattice l = out;
    l.x = hc.at<double>(o_x), l.y = hc.at<double>(o_y), l.stride = d_stride;
    if ((rc = warp_launch_status(hk::launch_warp_coords(warp, l, hc.sl.stream, &why), why))) return rc;
    if ((rc = stage_d2h(hc.sl, out.x, (size_t)out.stride * 8, l.x, (size_t)d_stride * 8, (size_t)out.w * 8, out.h))) return rc;
    if ((rc = stage_d2h(hc.sl, out.y, (size_t)out.stride * 8, l.y, (size_t)d_stride * 8, (size_t)out.w * 8, out.h))) return rc;
    return stage_finish(hc.sl);
}

int hk_warp_coords_dev(hk_ctx* ctx, const hk_warp_desc* warp, double off_row, double off_col, int32_t height, int32_t width,
                       double* x_dev, double* y_dev, int64_t stride, int32_t stream) {
    return warp_coords_dev(ctx, warp, {.x = x_dev, .y = y_dev, .stride = stride, .h = height, .w = width, .off_row = off_row, .off_col = off_col}, stream);
}

int hk_warp_coords(hk_ctx* ctx, const hk_warp_desc* warp, double off_row, double off_col, int32_t height, int32_t width,
                   double* x_out, double* y_out, int64_t stride) {
    return warp_coords_host(ctx, warp, {.x = x_out, .y = y_out, .stride = stride, .h = height, .w = width, .off_row = off_row, .off_col = off_col});
}

int hk_warp_coords_affine_dev(hk_ctx* ctx, const hk_affine_warp_desc* warp, double off_row, double off_col, int32_t height,
                              int32_t width, double* x_dev, double* y_dev, int64_t stride, int32_t stream) {
    return warp_coords_dev(ctx, warp, {.x = x_dev, .y = y_dev, .stride = stride, .h = height, .w = width, .off_row = off_row, .off_col = off_col}, stream);
}

int hk_warp_coords_affine(hk_ctx* ctx, const hk_affine_warp_desc* warp, double off_row, double off_col, int32_t height,
                          int32_t width, double* x_out, double* y_out, int64_t stride) {
    return warp_coords_host(ctx, warp, {.x = x_out, .y = y_out, .stride = stride, .h = height, .w = width, .off_row = off_row, .off_col = off_col});
}

static int check_reproject_crs(hk_ctx* ctx, const void* warp, bool affine, const hk::ResamplePlanes& p, double kx, double ky,
                               int32_t resampling) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!warp || !p.src || !p.dst) return null_arg();
    if (p.n_bands < 1 || p.sh < 1 || p.sw < 1 || p.dh < 1 || p.dw < 1) return fail(HK_ERR_ARG, "empty raster");
    if (!(kx > 0.0) || !(ky > 0.0) || !std::isfinite(kx) || !std::isfinite(ky))
        return fail(HK_ERR_ARG, "kx, ky must be positive and finite");
    if (!resampling_built(resampling))
        return fail(HK_ERR_UNSUPPORTED, "resampling %d is not a warp method", resampling);
    if (resampling > 4)
        return fail(HK_ERR_UNSUPPORTED, affine ? "resampling %d works on a destination pixel's footprint, which is not built between "
                                                 "rotated / sheared grids (nearest, bilinear, cubic, cubic_spline and lanczos are)"
                                               : "resampling %d works on a destination pixel's footprint, which is not built across CRSs "
                                                 "(nearest, bilinear, cubic, cubic_spline and lanczos are)", resampling);
    if (p.dh > 65535) return fail(HK_ERR_UNSUPPORTED, "destination taller than 65535 rows");
    return check_nodata_mode(p.nd_mode);
}

extern "C++" template <typename Desc>
static int reproject_warp_dev(hk_ctx* ctx, const Desc* warp, const hk::ResamplePlanes& p, double kx, double ky, int32_t resampling,
                              int32_t stream) {
    int rc = check_reproject_crs(ctx, warp, std::is_same<Desc, hk_affine_warp_desc>::value, p, kx, ky, resampling);
    if (rc) return rc;
    if ((rc = check_resample_strides(p)) || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    const char* why = nullptr;
    return warp_launch_status(hk::launch_warp_resample(resampling, warp, p, kx, ky, ctx->slots[stream].stream, &why), why);
}

extern "C++" template <typename Desc>
static int reproject_warp_host(hk_ctx* ctx, const Desc* warp, const hk::ResamplePlanes& p, double kx, double ky, int32_t resampling) {
    const int rc = check_reproject_crs(ctx, warp, std::is_same<Desc, hk_affine_warp_desc>::value, p, kx, ky, resampling);
    if (rc) return rc;
    return reproject_packed(ctx, p, [&](const hk::ResamplePlanes& slab, hipStream_t stream) {
        const char* why = nullptr;
        return warp_launch_status(hk::launch_warp_resample(resampling, warp, slab, kx, ky, stream, &why), why);
    });
}

int hk_reproject_crs_dev(hk_ctx* ctx, const hk_warp_desc* warp, const float* src_dev, int32_t n_bands, int32_t src_height,
                         int32_t src_width, int64_t src_stride, int64_t src_band_stride, int32_t src_nodata_mode,
                         float src_nodata, double kx, double ky, int32_t resampling, float* dst_dev, int32_t dst_height,
                         int32_t dst_width, int64_t dst_stride, int64_t dst_band_stride, float dst_fill, int32_t stream) {
    const hk::ResamplePlanes p = {.src = src_dev, .dst = dst_dev, .src_stride = src_stride, .src_band_stride = src_band_stride,
                                  .dst_stride = dst_stride, .dst_band_stride = dst_band_stride, .sh = src_height, .sw = src_width,
                                  .dh = dst_height, .dw = dst_width, .n_bands = n_bands, .nd_mode = src_nodata_mode, .nodata = src_nodata,
                                  .dst_fill = dst_fill};
    return reproject_warp_dev(ctx, warp, p, kx, ky, resampling, stream);
}

int hk_reproject_crs(hk_ctx* ctx, const hk_warp_desc* warp, const float* src, int32_t n_bands, int32_t src_height,
                     int32_t src_width, int32_t src_nodata_mode, float src_nodata, double kx, double ky, int32_t resampling,
                     float* dst, int32_t dst_height, int32_t dst_width, float dst_fill) {
    const hk::ResamplePlanes p = {.src = src, .dst = dst, .sh = src_height, .sw = src_width, .dh = dst_height, .dw = dst_width,
                                  .n_bands = n_bands, .nd_mode = src_nodata_mode, .nodata = src_nodata, .dst_fill = dst_fill};
    return reproject_warp_host(ctx, warp, p, kx, ky, resampling);
}

int hk_reproject_affine_dev(hk_ctx* ctx, const hk_affine_warp_desc* warp, const float* src_dev, int32_t n_bands,
                            int32_t src_height, int32_t src_width, int64_t src_stride, int64_t src_band_stride,
                            int32_t src_nodata_mode, float src_nodata, double kx, double ky, int32_t resampling, float* dst_dev,
                            int32_t dst_height, int32_t dst_width, int64_t dst_stride, int64_t dst_band_stride, float dst_fill,
                            int32_t stream) {
    const hk::ResamplePlanes p = {.src = src_dev, .dst = dst_dev, .src_stride = src_stride, .src_band_stride = src_band_stride,
                                  .dst_stride = dst_stride, .dst_band_stride = dst_band_stride, .sh = src_height, .sw = src_width,
                                  .dh = dst_height, .dw = dst_width, .n_bands = n_bands, .nd_mode = src_nodata_mode, .nodata = src_nodata,
                                  .dst_fill = dst_fill};
    return reproject_warp_dev(ctx, warp, p, kx, ky, resampling, stream);
}

int hk_reproject_affine(hk_ctx* ctx, const hk_affine_warp_desc* warp, const float* src, int32_t n_bands, int32_t src_height,
                        int32_t src_width, int32_t src_nodata_mode, float src_nodata, double kx, double ky, int32_t resampling,
                        float* dst, int32_t dst_height, int32_t dst_width, float dst_fill) {
    const hk::ResamplePlanes p = {.src = src, .dst = dst, .sh = src_height, .sw = src_width, .dh = dst_height, .dw = dst_width,
                                  .n_bands = n_bands, .nd_mode = src_nodata_mode, .nodata = src_nodata, .dst_fill = dst_fill};
    return reproject_warp_host(ctx, warp, p, kx, ky, resampling);
}

int hk_partial_mask(hk_ctx* ctx, const float* in, int64_t in_stride, int32_t in_nodata_mode, float in_nodata,
                    const float* params, int32_t n_param_bands, const float* src, int64_t src_stride, int32_t height,
                    int32_t width, int32_t kh, int32_t kw, float* params_out, float* corr_out, uint8_t* mask_out) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!in || !params) return null_arg();
    if (height < 1 || width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d", height, width);
    if (n_param_bands < 2 || n_param_bands > 3) return fail(HK_ERR_ARG, "params must have 2 or 3 bands");
    if (kh < 1 || kw < 1 || !(kh & 1) || !(kw & 1)) return fail(HK_ERR_ARG, "`kernel_shape` must be odd in both dimensions.");
    int rc = check_mask_kernel(kh, kw);
    if (rc) return rc;
    if (corr_out && !src) return fail(HK_ERR_ARG, "corr_out needs src");
    if ((rc = check_strides(in_stride, width)) || (src && (rc = check_strides(src_stride, width)))) return rc;
    if ((rc = check_nodata_mode(in_nodata_mode, hk::ND_COVERAGE))) return rc;  // (include/homonim_hk.h states it as 3)
    HK_ENTER(ctx);
    const int64_t stride = row_align(width);
    const size_t plane = (size_t)stride * height * sizeof(float);
    SlabLayout L;
    const size_t o_in = L.take(plane), o_par = L.take(plane * n_param_bands), o_src = src ? L.take(plane) : 0;
    const size_t o_pout = params_out ? L.take(plane * n_param_bands) : 0, o_corr = corr_out ? L.take(plane) : 0;
    const size_t o_mask = mask_out ? L.take((size_t)stride * height) : 0, o_cnt = L.take((size_t)stride * height * 2);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    float *d_in = hc.at<float>(o_in), *d_par = hc.at<float>(o_par), *d_src = src ? hc.at<float>(o_src) : nullptr;
    float *d_pout = params_out ? hc.at<float>(o_pout) : nullptr, *d_corr = corr_out ? hc.at<float>(o_corr) : nullptr;
    unsigned char* d_mask = mask_out ? hc.at<unsigned char>(o_mask) : nullptr;
    const size_t wb = (size_t)width * 4, sb = (size_t)stride * 4;
    if ((rc = stage_h2d(sl, d_in, sb, in, in_stride * 4, wb, height))) return rc;
    for (int b = 0; b < n_param_bands; ++b)
        if ((rc = stage_h2d(sl, d_par + (size_t)b * stride * height, sb, params + (size_t)b * height * width, wb, wb, height)))
            return rc;
    if (src && (rc = stage_h2d(sl, d_src, sb, src, src_stride * 4, wb, height))) return rc;
    HK_HIP(hk::launch_partial_mask({.in = d_in, .nd_mode = in_nodata_mode, .nodata = in_nodata, .params = d_par, .n_bands = n_param_bands,
                                    .band_stride = stride * height, .src = d_src, .height = height, .width = width, .stride = stride,
                                    .kh = kh, .kw = kw, .params_out = d_pout, .corr_out = d_corr, .mask_out = d_mask},
                                   hc.at<unsigned short>(o_cnt), sl.stream));
    if (params_out)
        for (int b = 0; b < n_param_bands; ++b)
            if ((rc = stage_d2h(sl, params_out + (size_t)b * height * width, wb, d_pout + (size_t)b * stride * height, sb, wb, height)))
                return rc;
    if (corr_out && (rc = stage_d2h(sl, corr_out, wb, d_corr, sb, wb, height))) return rc;
    if (mask_out && (rc = stage_d2h(sl, mask_out, width, d_mask, stride, width, height))) return rc;
    return stage_finish(sl);
}

// ---------------------------------------------------------------------------------------------------------------------
int hk_host_alloc(hk_ctx* ctx, size_t bytes, void** hptr) {
    if (!ctx || !hptr) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    if (hipHostMalloc(hptr, bytes, hipHostMallocPortable) != hipSuccess)
        return fail(HK_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes);
    pinned_ranges().add(*hptr, bytes);
    return HK_OK;
}
int hk_host_free(hk_ctx* ctx, void* hptr) {
    // page-locked host memory belongs to no device: `ctx` may be NULL (e.g. the context was destroyed first)
    (void)ctx;
    pinned_ranges().remove(hptr);
    HK_HIP(hipHostFree(hptr));
    return HK_OK;
}
int hk_host_register(hk_ctx* ctx, void* hptr, size_t bytes) {
    if (!ctx || !hptr) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    // page-locked already (hk_host_alloc, or somebody's registration)?  hipHostRegister answers that case with different
    // errors (AlreadyRegistered, InvalidValue for hipHostMalloc memory) or not at all, so ask first
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, hptr) == hipSuccess && attr.type == hipMemoryTypeHost)
        return fail(HK_ERR_ALREADY, "host memory is page-locked already");
    (void)hipGetLastError();  // pageable memory: the query itself may have failed
    hipError_t e = hipHostRegister(hptr, bytes, hipHostRegisterPortable);
    if (e == hipErrorHostMemoryAlreadyRegistered) {
        (void)hipGetLastError();
        return fail(HK_ERR_ALREADY, "host memory is page-locked already");
    }
    HK_HIP(e);
    pinned_ranges().add(hptr, bytes);
    return HK_OK;
}
int hk_host_unregister(hk_ctx* ctx, void* hptr) {
    if (!hptr) return fail(HK_ERR_ARG, "NULL argument");
    (void)ctx;  // may be NULL, like hk_host_free
    pinned_ranges().remove(hptr);
    HK_HIP(hipHostUnregister(hptr));
    return HK_OK;
}
int hk_debug_staging_counters(uint64_t out[2], int32_t reset) {
    if (!out) return fail(HK_ERR_ARG, "out is NULL");
    out[0] = g_direct_copies.load(), out[1] = g_staged_chunks.load();
    if (reset) g_direct_copies.store(0), g_staged_chunks.store(0);
    return HK_OK;
}

int hk_debug_fail_after_d2h(int32_t on) {
    g_fail_after_d2h.store(on != 0);
    return HK_OK;
}

int hk_debug_build_ledger(char* buf, size_t len, size_t* needed, int32_t reset) {
    const size_t n = hk::ledger_text(buf, buf ? len : 0, reset != 0);
    if (needed) *needed = n;
    if (buf && n > len) return fail(HK_ERR_ARG, "ledger needs %zu bytes, the buffer has %zu", n, len);
    return HK_OK;
}

int hk_debug_fit_build(const hk_fit_desc* desc, int32_t height, int32_t width, int32_t n_bands, uint32_t planes, int32_t phase,
                       int32_t force_ring, int32_t force_general, char* name, size_t len) {
    const int rc = validate_desc(desc);
    if (rc) return rc;
    if (!name || height < 1 || width < 1 || n_bands < 1 || planes > 255u || phase < 0 || phase > 2 || force_ring < -1 || force_ring > 3)
        return fail(HK_ERR_ARG, "hk_debug_fit_build: NULL name, empty job, or unknown planes / phase / ring");
    LaunchPolicy lp;
    lp.force_general = force_general != 0;
    if (force_ring >= 0) lp.use_ring = force_ring;
    float* const set = reinterpret_cast<float*>(sizeof(float4));  // (never read: the chooser asks which planes there are)
    auto plane = [&](unsigned bit) { return (planes & bit) ? set : nullptr; };
    hk::FitArgs a;
    memset(&a, 0, sizeof(a));
    a.gain = plane(1), a.offset = plane(2), a.r2 = plane(4), a.corr = plane(8), a.offset_in = plane(64);
    a.fail_count = reinterpret_cast<unsigned long long*>(plane(16)), a.flag = reinterpret_cast<unsigned char*>(plane(32));
    a.flag_in = a.offset_in ? reinterpret_cast<const unsigned char*>(set) : nullptr;
    a.jobs = reinterpret_cast<const hk::FitJob*>(plane(128));
    a.height = height, a.width = width, a.n_bands = n_bands;
    fill_args(a, desc, lp);
    const bool r2 = needs_r2(desc) && !a.offset_in;  // (the closing pass runs the build without the R2 work: inpaint_band)
    if (phase && !cert_list_eligible(a, desc, r2)) return fail(HK_ERR_ARG, "this launch has no certificate build + list launch");
    a.cert_only = phase == 1, a.list_mode = phase == 2;
    const hk::FitBuild b = hk::choose_fit_build(a, desc->model, r2);
    if (!hk::fit_build_exists(b)) return fail(HK_ERR_ARG, "this launch has no build of the fused kernel");
    hk::fit_build_name(name, len, b);
    return HK_OK;
}

int hk_dev_alloc(hk_ctx* ctx, size_t bytes, void** dptr) {
    if (!ctx || !dptr) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    if (dev_malloc(dptr, bytes) != hipSuccess) return fail(HK_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return HK_OK;
}
int hk_dev_free(hk_ctx* ctx, void* dptr) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    HK_ENTER(ctx);
    HK_HIP(dev_free(dptr));
    return HK_OK;
}
int hk_memcpy_h2d(hk_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!bytes) return HK_OK;
    if (!dst || !src) return null_arg();
    HK_ENTER(ctx);
    std::lock_guard<std::mutex> lk(ctx->xfer_mu);
    int rc = stage_h2d(ctx->xfer, dst, bytes, src, bytes, bytes, 1);
    if (!rc) rc = stage_finish(ctx->xfer);
    if (rc) stage_abandon(ctx->xfer);
    return rc;
}
int hk_memcpy_d2h(hk_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!bytes) return HK_OK;
    if (!dst || !src) return null_arg();
    HK_ENTER(ctx);
    std::lock_guard<std::mutex> lk(ctx->xfer_mu);
    int rc = stage_d2h(ctx->xfer, dst, bytes, src, bytes, bytes, 1);
    if (!rc) rc = stage_finish(ctx->xfer);
    if (rc) stage_abandon(ctx->xfer);   // (a second chunk that failed leaves the first one queued with the caller's pointer)
    return rc;
}
int hk_memset(hk_ctx* ctx, void* dst, int value, size_t bytes) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    HK_ENTER(ctx);
    HK_HIP(hipMemset(dst, value, bytes));
    return HK_OK;
}

// elements spanned by the job's planes (last band's plane included)
static size_t job_span(int32_t n_bands, int32_t height, int64_t stride, int64_t band_stride) {
    const size_t plane = (size_t)stride * (size_t)height;
    return n_bands > 1 ? (size_t)(n_bands - 1) * (size_t)band_stride + plane : plane;
}
uint64_t hk_dev_job_scratch_bytes(int32_t n_bands, int32_t height, int64_t stride, int64_t band_stride) {
    if (n_bands < 1 || height < 1 || stride < 1 || band_stride < 0) return 0;
    return (uint64_t)job_span(n_bands, height, stride, band_stride) * 5u;
}
// the job's scratch planes (NULL without scratch): offsets (float32) and source flags (1 byte), indexed like the job's planes
static float* job_scratch_offset(const hk_dev_job* job) { return static_cast<float*>(job->scratch); }
static unsigned char* job_scratch_flag(const hk_dev_job* job) {
    return job->scratch ? static_cast<unsigned char*>(job->scratch) +
                              4 * job_span(job->n_bands, job->height, job->stride, job->band_stride)
                        : nullptr;
}

static int check_job(hk_ctx* ctx, const hk_dev_job* job, bool allow_no_rows = false) {
    if (!ctx || !job) return fail(HK_ERR_ARG, "NULL argument");
    if (!job->src || !job->ref) return fail(HK_ERR_ARG, "job src/ref is NULL");
    if (job->n_bands < 1 || job->height < (allow_no_rows ? 0 : 1) || job->width < 1) return fail(HK_ERR_ARG, "empty job");
    if (job->stride < job->width || (job->stride % hk::PX) != 0)
        return fail(HK_ERR_ARG, "job stride must be >= width and a multiple of %d elements", hk::PX);
    if ((job->band_stride % hk::PX) != 0) return fail(HK_ERR_ARG, "band_stride must be a multiple of %d", hk::PX);
    if (((uintptr_t)job->src | (uintptr_t)job->ref | (uintptr_t)job->gain | (uintptr_t)job->offset |
         (uintptr_t)job->r2 | (uintptr_t)job->corr) & 15)
        return fail(HK_ERR_ARG, "device planes must be 16-byte aligned");
    if (const int bad = check_stream(ctx, job->stream)) return bad;
    if (job->scratch) {
        if ((uintptr_t)job->scratch & 15) return fail(HK_ERR_ARG, "job scratch must be 16-byte aligned");
        if (job->scratch_bytes < hk_dev_job_scratch_bytes(job->n_bands, job->height, job->stride, job->band_stride))
            return fail(HK_ERR_ARG, "job scratch smaller than hk_dev_job_scratch_bytes()");
    }
    if (job->out_rows || job->out_cols) {
        if (job->out_row0 < 0 || job->out_col0 < 0 || job->out_rows < 1 || job->out_cols < 1 ||
            job->out_row0 + job->out_rows > job->height || job->out_col0 + job->out_cols > job->width)
            return fail(HK_ERR_ARG, "job store window outside the job");
        if ((job->out_col0 % hk::PX) != 0 || (((job->out_col0 + job->out_cols) % hk::PX) != 0 && job->out_col0 + job->out_cols != job->width))
            return fail(HK_ERR_ARG, "job store window must start and end on multiples of %d columns (or at the job's last column)", hk::PX);
    }
    return HK_OK;
}

int hk_fit_apply_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_job(ctx, job);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (desc->model == HK_MODEL_GAIN_BLK_OFFSET && !job->norm) return fail(HK_ERR_ARG, "gain-blk-offset needs job->norm");
    HK_ENTER(ctx);
    hk::FitArgs a;
    if ((rc = job_fit_args(a, ctx, desc, *job))) return rc;
    if (desc->model == HK_MODEL_GAIN_OFFSET && a.has_thresh && job->scratch) {
        // a job that carries scratch gets the in-painting's inputs -- offsets + source flags, 5 bytes per pixel -- left there by
        // this pass (hk_inpaint_dev_counts starts from them): a caller that expects pixels to fail the r2 mask provides it
        a.flag = job_scratch_flag(job);
        if (!a.offset) a.offset = job_scratch_offset(job);
    }
    return launch_fit(ctx, ctx->slots[job->stream], a, desc, needs_r2(desc));
}

int hk_fail_counts_async(hk_ctx* ctx, const hk_dev_job* job, uint64_t* host_counts, hk_event* ready) {
    int rc = check_job(ctx, job);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (!job->fail_count || !host_counts || !ready) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    const size_t bytes = (size_t)job->n_bands * sizeof(unsigned long long);
    if (!host_is_pinned(host_counts, bytes)) return fail(HK_ERR_ARG, "host_counts must be page-locked memory (hk_host_alloc / hk_host_register)");
    HK_HIP(hipMemcpyAsync(host_counts, job->fail_count, bytes, hipMemcpyDeviceToHost, sl.stream));
    // the counters are consumed: the next hk_fit_apply_dev into this buffer starts from zero
    HK_HIP(hipMemsetAsync(job->fail_count, 0, bytes, sl.stream));
    HK_HIP(hipEventRecord(ready->ev, sl.stream));
    return HK_OK;
}

int hk_debug_stage_stamps(hk_ctx* ctx, uint64_t out[16], int32_t reset) {
    if (!ctx || !out) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    HK_HIP(hipDeviceSynchronize());
    unsigned long long tmp[16];
    HK_HIP(hk::read_stamps(tmp, reset != 0));
    for (int i = 0; i < 16; ++i) out[i] = tmp[i];
    return HK_OK;
}

int hk_r2_certificate_constants(float thresh, double* pass_below, double* fail_above, float* kappa, float* kappa_fail) {
    if (pass_below) *pass_below = r2_pass_scale(thresh);
    if (fail_above) *fail_above = r2_fail_above(thresh);
    if (kappa) *kappa = r2_fail_scale(thresh);
    if (kappa_fail) *kappa_fail = r2_failcert_scale(thresh);
    return HK_OK;
}

int hk_counts_pending(const uint64_t* counts, int32_t n_bands) {
    if (!counts) return 0;
    for (int32_t b = 0; b < n_bands; ++b)
        if (counts[b]) return 1;  // failing pixels
    return 0;
}

int hk_event_sync(hk_ctx* ctx, hk_event* ev) {
    if (!ctx || !ev) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    HK_HIP(hipEventSynchronize(ev->ev));
    return HK_OK;
}

int hk_inpaint_dev_counts(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, const uint64_t* counts,
                          uint64_t* n_fail_out) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_job(ctx, job);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (n_fail_out) *n_fail_out = 0;
    if (desc->model != HK_MODEL_GAIN_OFFSET || !desc->has_r2_thresh) return HK_OK;  // nothing to in-paint
    if (!counts) return fail(HK_ERR_ARG, "counts is NULL");
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    const bool r2 = needs_r2(desc);
    unsigned long long total = 0;
    for (int b = 0; b < job->n_bands; ++b) {
        unsigned long long n_fail = counts[b];
        if (n_fail == 0) continue;
        const long long off = (long long)b * job->band_stride;
        hk::FitArgs a;
        if ((rc = job_fit_args(a, ctx, desc, *job, b))) return rc;
        std::unique_lock<std::mutex> lk(ctx->mu);  // the slot's scratch may be (re)allocated
        // offsets + source flags left by the pass that counted, which writes them whenever the job carries scratch (hk_fit_apply_dev)
        InpaintInputs left = {};
        if (job->scratch) left = {a.offset ? a.offset : job_scratch_offset(job) + off, job_scratch_flag(job) + off};
        total += n_fail;
        rc = inpaint_band(sl, a, desc, r2, n_fail, job->scratch ? &left : nullptr);
        if (rc) return rc;
    }
    if (n_fail_out) *n_fail_out = total;
    return HK_OK;
}

int hk_inpaint_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, uint64_t* n_fail_out) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_job(ctx, job);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (n_fail_out) *n_fail_out = 0;
    if (desc->model != HK_MODEL_GAIN_OFFSET || !desc->has_r2_thresh) return HK_OK;  // nothing to in-paint
    if (!job->fail_count) return fail(HK_ERR_ARG, "job->fail_count is NULL");
    if (job->n_bands > 1024) return fail(HK_ERR_ARG, "too many bands");
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    std::vector<uint64_t> counts((size_t)job->n_bands);
    uint64_t* const pinned = sl.pin<uint64_t>(Slot::PIN_COUNTS);  // <= 1024 counters (checked above)
    HK_HIP(hipMemcpyAsync(pinned, job->fail_count, counts.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.stream));
    HK_HIP(hipStreamSynchronize(sl.stream));
    memcpy(counts.data(), pinned, counts.size() * sizeof(uint64_t));
    // the counters are consumed: the next hk_fit_apply_dev of this job starts from zero
    HK_HIP(hipMemsetAsync(job->fail_count, 0, counts.size() * sizeof(uint64_t), sl.stream));
    return hk_inpaint_dev_counts(ctx, desc, job, counts.data(), n_fail_out);
}

// Reduction workspace of the device-resident entry points on one stream (block statistics, comparison sums).
static int ensure_stream_ws(hk_ctx* ctx, Slot& sl, size_t need) {
    // device-resident jobs on one stream are issued by one caller at a time (stream order); the lock only protects
    // the (re)allocation against other streams' callers touching the context
    std::lock_guard<std::mutex> lk(ctx->mu);
    return grow_slot_buf(sl, sl.norm_ws, sl.norm_ws_bytes, need);
}

int hk_compare_sums_dev(hk_ctx* ctx, const hk_dev_job* job, int32_t src_nodata_mode, float src_nodata,
                        int32_t ref_nodata_mode, float ref_nodata, double* sums_dev) {
    int rc = check_job(ctx, job);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (!sums_dev) return fail(HK_ERR_ARG, "sums_dev is NULL");
    if ((rc = check_nodata_modes(src_nodata_mode, ref_nodata_mode))) return rc;
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    rc = ensure_stream_ws(ctx, sl, hk::compare_workspace_bytes(job->n_bands));
    if (rc) return rc;
    const hk::CompareArgs ca = {.src = job->src, .ref = job->ref, .height = job->height, .width = job->width, .src_stride = job->stride,
                                .ref_stride = job->stride, .src_band_stride = job->band_stride, .ref_band_stride = job->band_stride,
                                .n_bands = job->n_bands, .src_nd_mode = src_nodata_mode, .ref_nd_mode = ref_nodata_mode,
                                .src_nodata = src_nodata, .ref_nodata = ref_nodata};
    HK_HIP(hk::launch_compare_sums(ca, sl.norm_ws, sums_dev, sl.stream));
    return HK_OK;
}

int hk_compare_sums(hk_ctx* ctx, const float* src, int64_t src_stride, int32_t src_nodata_mode, float src_nodata,
                    const float* ref, int64_t ref_stride, int32_t ref_nodata_mode, float ref_nodata, int32_t height,
                    int32_t width, double sums_out[7]) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!src || !ref || !sums_out) return null_arg();
    if (height < 1 || width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d", height, width);
    int rc = check_strides(src_stride, width, ref_stride, width);
    if (rc || (rc = check_nodata_modes(src_nodata_mode, ref_nodata_mode))) return rc;
    HK_ENTER(ctx);
    const int64_t stride = row_align(width);
    const size_t plane = (size_t)stride * height * sizeof(float);
    SlabLayout L;
    const size_t o_src = L.take(plane), o_ref = L.take(plane), o_ws = L.take(hk::compare_workspace_bytes(1)), o_sums = L.take(256);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    float *d_src = hc.at<float>(o_src), *d_ref = hc.at<float>(o_ref);
    double* d_sums = hc.at<double>(o_sums);
    const size_t wbytes = (size_t)width * sizeof(float);
    if ((rc = stage_h2d(hc.sl, d_src, stride * 4, src, src_stride * 4, wbytes, height))) return rc;
    if ((rc = stage_h2d(hc.sl, d_ref, stride * 4, ref, ref_stride * 4, wbytes, height))) return rc;
    const hk::CompareArgs ca = {.src = d_src, .ref = d_ref, .height = height, .width = width, .src_stride = stride, .ref_stride = stride,
                                .n_bands = 1, .src_nd_mode = src_nodata_mode, .ref_nd_mode = ref_nodata_mode, .src_nodata = src_nodata,
                                .ref_nodata = ref_nodata};
    HK_HIP(hk::launch_compare_sums(ca, hc.at(o_ws), d_sums, hc.sl.stream));
    HK_HIP(hipMemcpyAsync(hc.sl.pin<double>(Slot::PIN_SUMS), d_sums, 7 * sizeof(double), hipMemcpyDeviceToHost, hc.sl.stream));
    if ((rc = stage_finish(hc.sl))) return rc;
    memcpy(sums_out, hc.sl.pin<double>(Slot::PIN_SUMS), 7 * sizeof(double));
    return HK_OK;
}

// ParamStats.stats / get_block_sums (homonim/stats.py:217-229): see include/homonim_hk.h
static int check_param_stats(hk_ctx* ctx, const hk::ParamStatsArgs& pa, const void* out) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!pa.planes || !out) return null_arg();
    if (pa.n_bands < 1 || pa.height < 1 || pa.width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d x %d", pa.n_bands, pa.height, pa.width);
    if (pa.n_bands > 65535) return fail(HK_ERR_ARG, "too many bands for one launch (%d > 65535)", pa.n_bands);
    const int rc = check_strides(pa.stride, pa.width);
    return rc ? rc : check_nodata_mode(pa.nd_mode);
}

int hk_param_stats_dev(hk_ctx* ctx, const float* planes_dev, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                       int64_t band_stride, int32_t stream, int32_t nodata_mode, float nodata, double thresh, double* stats_dev) {
    const hk::ParamStatsArgs pa = {.planes = planes_dev, .height = height, .width = width, .stride = stride, .band_stride = band_stride,
                                   .n_bands = n_bands, .nd_mode = nodata_mode, .nodata = nodata, .thresh = thresh};
    int rc = check_param_stats(ctx, pa, stats_dev);
    if (rc || (rc = check_band_strides(band_stride)) || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[stream];
    rc = ensure_stream_ws(ctx, sl, hk::param_stats_workspace_bytes(n_bands));
    if (rc) return rc;
    HK_HIP(hk::launch_param_stats(pa, sl.norm_ws, stats_dev, sl.stream));
    return HK_OK;
}

int hk_param_stats(hk_ctx* ctx, const float* plane, int64_t stride, int32_t nodata_mode, float nodata, double thresh,
                   int32_t height, int32_t width, double stats_out[10]) {
    static_assert(hk::PARAM_STATS_N == 10, "stats_out[10] of include/homonim_hk.h");
    hk::ParamStatsArgs pa = {.planes = plane, .height = height, .width = width, .stride = stride, .n_bands = 1, .nd_mode = nodata_mode,
                             .nodata = nodata, .thresh = thresh};
    int rc = check_param_stats(ctx, pa, stats_out);
    if (rc) return rc;
    HK_ENTER(ctx);
    const int64_t d_stride = row_align(width);
    SlabLayout L;
    const size_t o_plane = L.take((size_t)d_stride * height * sizeof(float)), o_ws = L.take(hk::param_stats_workspace_bytes(1)),
                 o_stats = L.take(256);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    float* d_plane = hc.at<float>(o_plane);
    double* d_stats = hc.at<double>(o_stats);
    if ((rc = stage_h2d(hc.sl, d_plane, d_stride * 4, plane, stride * 4, (size_t)width * sizeof(float), height))) return rc;
    pa.planes = d_plane, pa.stride = d_stride;  // the plane in the slab
    HK_HIP(hk::launch_param_stats(pa, hc.at(o_ws), d_stats, hc.sl.stream));
    const size_t bytes = hk::PARAM_STATS_N * sizeof(double);
    HK_HIP(hipMemcpyAsync(hc.sl.pin<double>(Slot::PIN_STATS), d_stats, bytes, hipMemcpyDeviceToHost, hc.sl.stream));
    if ((rc = stage_finish(hc.sl))) return rc;
    memcpy(stats_out, hc.sl.pin<double>(Slot::PIN_STATS), bytes);
    return HK_OK;
}

// Internal overviews (homonim/fuse.py:152-165): see include/homonim_hk.h
int hk_overview_count(int32_t height, int32_t width, int32_t* n) {
    if (!n) return fail(HK_ERR_ARG, "n is NULL");
    if (height < 1 || width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d", height, width);
    int lg = 0;  // int(min(log2(height), log2(width)))
    for (int32_t m = height < width ? height : width; m > 1; m >>= 1) ++lg;
    *n = lg - 8 < 0 ? 0 : (lg - 8 > 8 ? 8 : lg - 8);
    return HK_OK;
}

constexpr int OVERVIEW_MAX_LEVELS = 31;

static_assert(sizeof(long long) == sizeof(int64_t), "strides, offsets and sizes of the ABI are handed on as they are");

static int check_overviews(hk_ctx* ctx, int32_t dtype, const hk::OverviewLevels& r) {
    const hk::BandPlanes& p = r.planes;
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!p.src || !r.out || !r.out_stride || !r.out_band_stride) return null_arg();
    if (!hk::dtype_size(dtype)) return fail(HK_ERR_ARG, "bad dtype %d", dtype);
    if (p.n_bands < 1 || p.height < 1 || p.width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d x %d", p.n_bands, p.height, p.width);
    if (p.n_bands > 65535) return fail(HK_ERR_ARG, "too many bands for one launch (%d > 65535)", p.n_bands);
    int rc = check_strides(p.stride, p.width);
    if (rc || (rc = check_band_strides(p.band_stride))) return rc;
    if (r.n_levels < 1 || r.n_levels > OVERVIEW_MAX_LEVELS) return fail(HK_ERR_ARG, "n_levels %d outside 1..%d", r.n_levels, OVERVIEW_MAX_LEVELS);
    for (int m = 1; m <= r.n_levels; ++m) {
        const int64_t wm = ((int64_t)p.width + (1ll << m) - 1) >> m;
        if (!r.out[m - 1]) return fail(HK_ERR_ARG, "level %d: NULL plane", m);
        if (r.out_stride[m - 1] < wm) return fail(HK_ERR_ARG, "level %d: row stride smaller than its width %lld", m, (long long)wm);
        if (r.out_band_stride[m - 1] < 0) return fail(HK_ERR_ARG, "level %d: band_stride is negative", m);
    }
    if ((rc = check_nodata_mode(r.nd_mode))) return rc;
    if (r.nd_mode == HK_NODATA_VALUE && dtype != HK_DTYPE_F32 && dtype != HK_DTYPE_F64 && !int_sample_holds(dtype, r.nodata))
        return fail(HK_ERR_ARG, "nodata %g is not a value of the integer sample type", r.nodata);
    return HK_OK;
}
// ... and of the masked forms: the raster's validity plane and one validity plane per level, strides in bytes
static int check_overviews_valid(hk_ctx* ctx, int32_t dtype, const hk::OverviewLevels& r) {
    int rc = check_overviews(ctx, dtype, r);
    if (rc) return rc;
    if (!r.valid || !r.out_valid || !r.out_valid_stride) return null_arg();
    if ((rc = check_strides(r.valid_stride, r.planes.width))) return rc;
    for (int m = 1; m <= r.n_levels; ++m) {
        const int64_t wm = ((int64_t)r.planes.width + (1ll << m) - 1) >> m;
        if (!r.out_valid[m - 1]) return fail(HK_ERR_ARG, "level %d: NULL validity plane", m);
        if (r.out_valid_stride[m - 1] < wm) return fail(HK_ERR_ARG, "level %d: validity row stride smaller than its width %lld", m, (long long)wm);
    }
    return HK_OK;
}

int hk_overviews_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                     int64_t stride, int64_t band_stride, int32_t nodata_mode, double nodata, int32_t n_levels,
                     void* const out_dev[], const int64_t out_stride[], const int64_t out_band_stride[], int32_t stream) {
    const hk::OverviewLevels r = {.planes = {.src = planes_dev, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                             .band_stride = band_stride},
                                  .nd_mode = nodata_mode, .nodata = nodata, .n_levels = n_levels, .out = out_dev,
                                  .out_stride = reinterpret_cast<const long long*>(out_stride),
                                  .out_band_stride = reinterpret_cast<const long long*>(out_band_stride)};
    int rc = check_overviews(ctx, dtype, r);
    if (rc || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    HK_HIP(hk::launch_overviews(dtype, r, ctx->slots[stream].stream));
    return HK_OK;
}

int hk_overviews_valid_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                           int64_t stride, int64_t band_stride, const uint8_t* valid_dev, int64_t valid_stride, int32_t n_levels,
                           void* const out_dev[], const int64_t out_stride[], const int64_t out_band_stride[],
                           uint8_t* const out_valid_dev[], const int64_t out_valid_stride[], int32_t stream) {
    const hk::OverviewLevels r = {.planes = {.src = planes_dev, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                             .band_stride = band_stride},
                                  .nd_mode = HK_NODATA_NONE, .nodata = 0., .n_levels = n_levels, .out = out_dev,
                                  .out_stride = reinterpret_cast<const long long*>(out_stride),
                                  .out_band_stride = reinterpret_cast<const long long*>(out_band_stride), .valid = valid_dev,
                                  .valid_stride = valid_stride, .out_valid = out_valid_dev,
                                  .out_valid_stride = reinterpret_cast<const long long*>(out_valid_stride)};
    int rc = check_overviews_valid(ctx, dtype, r);
    if (rc || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    HK_HIP(hk::launch_overviews(dtype, r, ctx->slots[stream].stream));
    return HK_OK;
}

// rows of source per strip of the host path: a multiple of 2^n_levels (cells of no level straddle two strips, so the strips are
// independent and their size cannot change a bit), all bands of at most OVERVIEW_STRIP_BYTES; HK_OVERVIEW_STRIP_KB (read at every
// call) lowers the bound for tests of the strip path
constexpr size_t OVERVIEW_STRIP_BYTES = 64u << 20;
static int64_t overview_strip_rows(int32_t n_bands, int32_t height, int32_t width, int esize, int32_t n_levels) {
    if (n_levels >= 31 || ((int64_t)1 << n_levels) >= height) return height;
    const size_t cap = cap_from_env("HK_OVERVIEW_STRIP_KB", OVERVIEW_STRIP_BYTES);
    const int64_t unit = (int64_t)1 << n_levels;
    const int64_t rows = (int64_t)(cap / ((size_t)n_bands * width * esize)) / unit * unit;
    return rows < unit ? unit : rows;
}

// The body of hk_overviews and hk_overviews_valid: `host` names the caller's arrays, with host.valid the masked form
static int overviews_host(hk_ctx* ctx, int32_t dtype, const hk::OverviewLevels& host) {
    const void* planes = host.planes.src;
    const int32_t n_bands = host.planes.n_bands, height = host.planes.height, width = host.planes.width, n_levels = host.n_levels;
    const int64_t stride = host.planes.stride, band_stride = host.planes.band_stride;
    void* const* out = host.out;
    const long long *out_stride = host.out_stride, *out_band_stride = host.out_band_stride;
    const bool masked = host.valid != nullptr;
    int rc = masked ? check_overviews_valid(ctx, dtype, host) : check_overviews(ctx, dtype, host);
    if (rc) return rc;
    HK_ENTER(ctx);
    const size_t es = hk::dtype_size(dtype);
    const int64_t strip = overview_strip_rows(n_bands, height, width, (int)es, n_levels);
    const int64_t rows_max = strip < height ? strip : height;
    auto ceil_shift = [](int64_t v, int m) { return (v + ((int64_t)1 << m) - 1) >> m; };
    // device slab of one strip: the source planes, then every level's planes, rows padded to ROW_ALIGN elements
    SlabLayout L;
    const int64_t d_stride = row_align(width);
    const size_t o_src = L.take((size_t)n_bands * rows_max * d_stride * es);
    size_t o_lev[OVERVIEW_MAX_LEVELS];
    long long l_stride[OVERVIEW_MAX_LEVELS], l_band[OVERVIEW_MAX_LEVELS];
    for (int m = 1; m <= n_levels; ++m) {
        l_stride[m - 1] = row_align(ceil_shift(width, m));
        l_band[m - 1] = l_stride[m - 1] * ceil_shift(rows_max, m);
        o_lev[m - 1] = L.take((size_t)n_bands * l_band[m - 1] * es);
    }
    // ... and in the masked form the strip's validity plane and every level's, one byte per pixel on the same row strides
    const size_t o_val = masked ? L.take((size_t)rows_max * d_stride) : 0;
    size_t o_lval[OVERVIEW_MAX_LEVELS];
    for (int m = 1; masked && m <= n_levels; ++m) o_lval[m - 1] = L.take((size_t)l_band[m - 1]);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    char* const base = hc.at(0);
    void* d_out[OVERVIEW_MAX_LEVELS];
    unsigned char* d_out_valid[OVERVIEW_MAX_LEVELS];
    for (int m = 1; m <= n_levels; ++m) d_out[m - 1] = base + o_lev[m - 1];
    for (int m = 1; masked && m <= n_levels; ++m) d_out_valid[m - 1] = reinterpret_cast<unsigned char*>(base + o_lval[m - 1]);
    const char* h_src = static_cast<const char*>(planes);
    for (int64_t r0 = 0; r0 < height; r0 += strip) {
        const int64_t rows = std::min<int64_t>(strip, height - r0);
        for (int b = 0; b < n_bands; ++b)
            if ((rc = stage_h2d(sl, base + o_src + (size_t)b * rows_max * d_stride * es, d_stride * es,
                                h_src + ((size_t)b * band_stride + (size_t)r0 * stride) * es, stride * es, (size_t)width * es, rows)))
                return rc;
        if (masked && (rc = stage_h2d(sl, base + o_val, d_stride, host.valid + (size_t)r0 * host.valid_stride, host.valid_stride, width, rows)))
            return rc;
        hk::OverviewLevels slab = host;  // this strip on the device
        slab.planes = {.src = base + o_src, .n_bands = n_bands, .height = (int)rows, .width = width, .stride = d_stride,
                       .band_stride = rows_max * d_stride};
        slab.out = d_out, slab.out_stride = l_stride, slab.out_band_stride = l_band;
        if (masked) {
            slab.valid = reinterpret_cast<const unsigned char*>(base + o_val), slab.valid_stride = d_stride;
            slab.out_valid = d_out_valid, slab.out_valid_stride = l_stride;
        }
        HK_HIP(hk::launch_overviews(dtype, slab, sl.stream));
        for (int m = 1; m <= n_levels; ++m) {
            char* h_out = static_cast<char*>(out[m - 1]);
            for (int b = 0; b < n_bands; ++b)
                if ((rc = stage_d2h(sl, h_out + ((size_t)b * out_band_stride[m - 1] + (size_t)(r0 >> m) * out_stride[m - 1]) * es,
                                    out_stride[m - 1] * es, base + o_lev[m - 1] + (size_t)b * l_band[m - 1] * es,
                                    l_stride[m - 1] * es, (size_t)ceil_shift(width, m) * es, ceil_shift(rows, m))))
                    return rc;
            if (masked && (rc = stage_d2h(sl, host.out_valid[m - 1] + (size_t)(r0 >> m) * host.out_valid_stride[m - 1],
                                          host.out_valid_stride[m - 1], d_out_valid[m - 1], l_stride[m - 1], ceil_shift(width, m),
                                          ceil_shift(rows, m))))
                return rc;
        }
    }
    return stage_finish(sl);
}

int hk_overviews(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                 int64_t band_stride, int32_t nodata_mode, double nodata, int32_t n_levels, void* const out[],
                 const int64_t out_stride[], const int64_t out_band_stride[]) {
    return overviews_host(ctx, dtype, {.planes = {.src = planes, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                                  .band_stride = band_stride},
                                       .nd_mode = nodata_mode, .nodata = nodata, .n_levels = n_levels, .out = out,
                                       .out_stride = reinterpret_cast<const long long*>(out_stride),
                                       .out_band_stride = reinterpret_cast<const long long*>(out_band_stride)});
}

int hk_overviews_valid(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                       int64_t band_stride, const uint8_t* valid, int64_t valid_stride, int32_t n_levels, void* const out[],
                       const int64_t out_stride[], const int64_t out_band_stride[], uint8_t* const out_valid[],
                       const int64_t out_valid_stride[]) {
    if (!valid) return null_arg();
    return overviews_host(ctx, dtype, {.planes = {.src = planes, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                                  .band_stride = band_stride},
                                       .nd_mode = HK_NODATA_NONE, .nodata = 0., .n_levels = n_levels, .out = out,
                                       .out_stride = reinterpret_cast<const long long*>(out_stride),
                                       .out_band_stride = reinterpret_cast<const long long*>(out_band_stride), .valid = valid,
                                       .valid_stride = valid_stride, .out_valid = out_valid,
                                       .out_valid_stride = reinterpret_cast<const long long*>(out_valid_stride)});
}

// The per-dataset mask of a GeoTIFF applied to its bands (hk_dataset_mask.hip): see include/homonim_hk.h
static int check_dataset_mask(hk_ctx* ctx, int32_t dtype, const hk::DatasetMask& a) {
    const hk::BandPlanes& p = a.planes;
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!p.src) return fail(HK_ERR_ARG, "planes is NULL");
    if (!a.mask) return fail(HK_ERR_ARG, "mask is NULL");
    if (!a.out) return fail(HK_ERR_ARG, "out is NULL");
    if (!hk::dtype_size(dtype)) return fail(HK_ERR_ARG, "bad dtype %d", dtype);
    if (a.kind != HK_MASK_BITS && a.kind != HK_MASK_ALPHA)
        return fail(HK_ERR_ARG, "bad mask_kind %d: %d (bits) or %d (alpha)", a.kind, HK_MASK_BITS, HK_MASK_ALPHA);
    if (a.kind == HK_MASK_ALPHA && dtype != HK_DTYPE_U8 && dtype != HK_DTYPE_U16)
        return fail(HK_ERR_ARG, "mask_kind alpha takes dtype uint8 or uint16, not dtype %d", dtype);
    if (p.n_bands < 1) return fail(HK_ERR_ARG, "n_bands %d is below 1", p.n_bands);
    if (p.height < 1) return fail(HK_ERR_ARG, "height %d is below 1", p.height);
    if (p.width < 1) return fail(HK_ERR_ARG, "width %d is below 1", p.width);
    if (p.stride < p.width) return fail(HK_ERR_ARG, "stride %lld is smaller than the width %d", p.stride, p.width);
    if (a.out_stride < p.width) return fail(HK_ERR_ARG, "out_stride %lld is smaller than the width %d", a.out_stride, p.width);
    const long long mask_min = a.kind == HK_MASK_BITS ? ((long long)p.width + 7) / 8 : (long long)p.width;
    if (a.mask_stride < mask_min)
        return fail(HK_ERR_ARG, "mask_stride %lld is smaller than the %lld %s of a mask row", a.mask_stride, mask_min,
                    a.kind == HK_MASK_BITS ? "bytes" : "samples");
    return HK_OK;
}

int hk_dataset_mask_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                        int64_t stride, int64_t band_stride, const void* mask_dev, int32_t mask_kind, int64_t mask_stride,
                        float* out_dev, int64_t out_stride, int64_t out_band_stride, int32_t stream) {
    const hk::DatasetMask a = {.planes = {.src = planes_dev, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                          .band_stride = band_stride},
                               .mask = mask_dev, .kind = mask_kind, .mask_stride = mask_stride, .out = out_dev, .out_stride = out_stride,
                               .out_band_stride = out_band_stride};
    int rc = check_dataset_mask(ctx, dtype, a);
    if (rc || (rc = check_band_strides(band_stride, out_band_stride)) || (rc = check_stream(ctx, stream))) return rc;
    const uintptr_t es = hk::dtype_size(dtype);
    if (reinterpret_cast<uintptr_t>(planes_dev) % es || (reinterpret_cast<uintptr_t>(out_dev) & 3u) ||
        (mask_kind == HK_MASK_ALPHA && reinterpret_cast<uintptr_t>(mask_dev) % es))
        return fail(HK_ERR_ARG, "planes_dev / mask_dev / out_dev: not aligned to the sample size");
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    HK_HIP(hk::launch_dataset_mask(dtype, a, ctx->slots[stream].stream));
    return HK_OK;
}

// The resident rasters of RasterFuse.process (hk_convert.hip): see include/homonim_hk.h
static int check_planes(const char* what, const void* p, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                        int64_t band_stride) {
    if (!p) return fail(HK_ERR_ARG, "%s is NULL", what);
    if (n_bands < 1 || height < 1 || width < 1) return fail(HK_ERR_ARG, "%s: empty raster %d x %d x %d", what, n_bands, height, width);
    if (stride < width) return fail(HK_ERR_ARG, "%s: stride %lld is smaller than the width %d", what, (long long)stride, width);
    if (band_stride < 0) return fail(HK_ERR_ARG, "%s: band_stride is negative", what);
    if (n_bands > 1 && band_stride < ((int64_t)height - 1) * stride + width)
        return fail(HK_ERR_ARG, "%s: band stride smaller than a plane: the planes overlap", what);
    if (reinterpret_cast<uintptr_t>(p) % (uintptr_t)hk::dtype_size(dtype)) return fail(HK_ERR_ARG, "%s: not aligned to the sample size", what);
    return HK_OK;
}
static int check_sample_value(int32_t dtype, double value, bool nan_allowed) {
    if (dtype == HK_DTYPE_F64) return (nan_allowed || value == value) ? HK_OK : fail(HK_ERR_ARG, "NaN is not a sample value here");
    if (dtype == HK_DTYPE_F32) {
        if (value != value) return nan_allowed ? HK_OK : fail(HK_ERR_ARG, "NaN is not a sample value here");
        return (!std::isfinite(value) || std::fabs(value) < 0x1.ffffffp127) ? HK_OK : fail(HK_ERR_ARG, "value %.17g is not a float32", value);
    }
    return int_sample_holds(dtype, value) ? HK_OK : fail(HK_ERR_ARG, "value %.17g is not a value of the integer sample type", value);
}

int hk_fill_planes_dev(hk_ctx* ctx, void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                       int64_t band_stride, double value, int32_t stream) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!hk::dtype_size(dtype)) return fail(HK_ERR_ARG, "bad dtype %d", dtype);
    int rc = check_planes("planes_dev", planes_dev, dtype, n_bands, height, width, stride, band_stride);
    if (rc || (rc = check_sample_value(dtype, value, true)) || (rc = check_stream(ctx, stream))) return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    HK_HIP(hk::launch_fill_planes(dtype, {.out = planes_dev, .stride = stride, .band_stride = band_stride, .n_bands = n_bands,
                                          .height = height, .width = width, .value = value}, ctx->slots[stream].stream));
    return HK_OK;
}

int hk_boundless_window_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                            int64_t stride, int64_t band_stride, int32_t row_off, int32_t col_off, int32_t out_height,
                            int32_t out_width, int32_t nodata_mode, double nodata, void* out_dev, int64_t out_stride,
                            int64_t out_band_stride, int32_t stream) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!hk::dtype_size(dtype)) return fail(HK_ERR_ARG, "bad dtype %d", dtype);
    int rc = check_nodata_mode(nodata_mode);
    if (rc) return rc;
    const bool to_float = nodata_mode != HK_NODATA_VALUE;
    if ((rc = check_planes("planes_dev", planes_dev, dtype, n_bands, height, width, stride, band_stride)) ||
        (rc = check_planes("out_dev", out_dev, to_float ? HK_DTYPE_F32 : dtype, n_bands, out_height, out_width, out_stride, out_band_stride)) ||
        (!to_float && (rc = check_sample_value(dtype, nodata, false))) || (rc = check_stream(ctx, stream)))
        return rc;
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    HK_HIP(hk::launch_boundless_window(dtype, {.in = planes_dev, .in_stride = stride, .in_band_stride = band_stride, .n_bands = n_bands,
                                               .height = height, .width = width, .row_off = row_off, .col_off = col_off,
                                               .out_height = out_height, .out_width = out_width, .to_float = to_float,
                                               .fill = to_float ? 0. : nodata, .out = out_dev, .out_stride = out_stride,
                                               .out_band_stride = out_band_stride}, ctx->slots[stream].stream));
    return HK_OK;
}

int hk_dev_mem_info(hk_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    HK_ENTER(ctx);
    size_t f = 0, t = 0;
    HK_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return HK_OK;
}

// device bytes of one chunk of the host path (rows are independent: the chunking cannot change a bit)
constexpr size_t DATASET_MASK_CHUNK_BYTES = 64u << 20;

int hk_dataset_mask(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                    const void* mask, int32_t mask_kind, int64_t mask_stride, float* out, int64_t out_stride) {
    // (the caller's bands lie `height` rows apart on both sides: the band strides are not read)
    const hk::DatasetMask host = {.planes = {.src = planes, .n_bands = n_bands, .height = height, .width = width, .stride = stride},
                                  .mask = mask, .kind = mask_kind, .mask_stride = mask_stride, .out = out, .out_stride = out_stride};
    int rc = check_dataset_mask(ctx, dtype, host);
    if (rc) return rc;
    HK_ENTER(ctx);
    const size_t es = hk::dtype_size(dtype);
    // device rows: samples and results padded to ROW_ALIGN elements, a row of mask bits to 16 bytes: every row may go wide
    const int64_t d_stride = row_align(width);
    const size_t ms = mask_kind == HK_MASK_BITS ? 1 : es;   // bytes per unit of mask_stride
    const int64_t d_mstride = mask_kind == HK_MASK_BITS ? (((int64_t)width + 7) / 8 + 15) / 16 * 16 : d_stride;
    const size_t m_row = mask_kind == HK_MASK_BITS ? (size_t)(((int64_t)width + 7) / 8) : (size_t)width * es;
    // whole rows per chunk: samples, mask and results of all bands within DATASET_MASK_CHUNK_BYTES (at least one row);
    // HK_STAGE_CHUNK_KB (read at every call here) lowers the bound for tests of the chunked path
    const size_t cap = cap_from_env("HK_STAGE_CHUNK_KB", DATASET_MASK_CHUNK_BYTES);
    const size_t per_row = (size_t)n_bands * d_stride * (es + sizeof(float)) + (size_t)d_mstride * ms;
    const int64_t rows_max = std::max<int64_t>(1, std::min<int64_t>(height, (int64_t)(cap / per_row)));
    SlabLayout L;
    const size_t o_in = L.take((size_t)n_bands * rows_max * d_stride * es), o_mask = L.take((size_t)rows_max * d_mstride * ms),
                 o_out = L.take((size_t)n_bands * rows_max * d_stride * sizeof(float));
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    char* const base = hc.at(0);
    const char *h_in = static_cast<const char*>(planes), *h_mask = static_cast<const char*>(mask);
    for (int64_t r0 = 0; r0 < height; r0 += rows_max) {
        const int64_t rows = std::min<int64_t>(rows_max, height - r0);
        for (int b = 0; b < n_bands; ++b)
            if ((rc = stage_h2d(sl, base + o_in + (size_t)b * rows_max * d_stride * es, d_stride * es,
                                h_in + ((size_t)b * height + (size_t)r0) * stride * es, stride * es, (size_t)width * es, rows)))
                return rc;
        if ((rc = stage_h2d(sl, base + o_mask, d_mstride * ms, h_mask + (size_t)r0 * mask_stride * ms, mask_stride * ms, m_row, rows))) return rc;
        const hk::DatasetMask slab = {.planes = {.src = base + o_in, .n_bands = n_bands, .height = (int)rows, .width = width, .stride = d_stride,
                                                 .band_stride = rows_max * d_stride},
                                      .mask = base + o_mask, .kind = mask_kind, .mask_stride = d_mstride, .out = hc.at<float>(o_out),
                                      .out_stride = d_stride, .out_band_stride = rows_max * d_stride};
        HK_HIP(hk::launch_dataset_mask(dtype, slab, sl.stream));
        for (int b = 0; b < n_bands; ++b)
            if ((rc = stage_d2h(sl, out + ((size_t)b * height + (size_t)r0) * out_stride, out_stride * sizeof(float),
                                hc.at<float>(o_out) + (size_t)b * rows_max * d_stride, d_stride * sizeof(float),
                                (size_t)width * sizeof(float), rows)))
                return rc;
    }
    return stage_finish(sl);
}

// DEFLATE streams of a raster's tiles (hk_deflate.hip): see include/homonim_hk.h
static int deflate_shape(int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int32_t tile, int64_t* n_tiles, int64_t* bytes,
                         int64_t* n_chunks) {
    const int es = hk::dtype_size(dtype);
    if (!es) return fail(HK_ERR_ARG, "bad dtype %d", dtype);
    if (n_bands < 1 || height < 1 || width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d x %d", n_bands, height, width);
    if (tile < 16 || tile > 512 || tile % 16) return fail(HK_ERR_ARG, "tile %d is not a multiple of 16 in 16..512", tile);
    const int64_t across = ((int64_t)width + tile - 1) / tile, down = ((int64_t)height + tile - 1) / tile;
    const int64_t raw = (int64_t)tile * tile * es, cpt = (raw + HK_DEFLATE_CHUNK - 1) / HK_DEFLATE_CHUNK;
    const int64_t per_tile = 2 + raw + 5 * cpt + 6;   // header, every chunk stored, final block and Adler-32
    *n_tiles = (int64_t)n_bands * across * down;
    *bytes = *n_tiles * (per_tile + (per_tile & 1));
    if (n_chunks) *n_chunks = *n_tiles * cpt;
    return HK_OK;
}

int hk_deflate_bound(int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int32_t tile, int64_t* n_tiles, int64_t* bytes) {
    if (!n_tiles || !bytes) return null_arg();
    return deflate_shape(dtype, n_bands, height, width, tile, n_tiles, bytes, nullptr);
}

// the predictor of hk_deflate_tiles_pred / _pred_dev against the dtype: 2 differences integers, 3 is the floating-point predictor
static int check_predictor(int32_t dtype, int32_t predictor) {
    if (predictor < 1 || predictor > 3) return fail(HK_ERR_ARG, "predictor %d is not 1, 2 or 3", predictor);
    if (!hk::dtype_size(dtype)) return fail(HK_ERR_ARG, "bad dtype %d", dtype);
    const bool is_float = dtype == HK_DTYPE_F32 || dtype == HK_DTYPE_F64;
    if (predictor == 2 && is_float) return fail(HK_ERR_ARG, "predictor 2 (horizontal differencing) is for integer samples, not dtype %d", dtype);
    if (predictor == 3 && !is_float) return fail(HK_ERR_ARG, "predictor 3 (floating point) is for float samples, not dtype %d", dtype);
    return HK_OK;
}

// (r.esize is not read: the dtype says it, and the dtype may be a bad one)
static int check_deflate(hk_ctx* ctx, int32_t dtype, const hk::DeflateTiles& r, int64_t out_capacity, int64_t* n_tiles, int64_t* n_chunks) {
    const hk::BandPlanes& p = r.planes;
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (!p.src || !r.out || !r.tile_offsets || !r.tile_sizes) return null_arg();
    int64_t bytes = 0;
    int rc = deflate_shape(dtype, p.n_bands, p.height, p.width, r.tile, n_tiles, &bytes, n_chunks);
    if (rc || (rc = check_strides(p.stride, p.width)) || (rc = check_band_strides(p.band_stride))) return rc;
    if (out_capacity < bytes) return fail(HK_ERR_ARG, "out_capacity %lld is below hk_deflate_bound's %lld", (long long)out_capacity, (long long)bytes);
    return HK_OK;
}

// the body of hk_deflate_tiles_dev and hk_deflate_tiles_pred_dev (which has checked the predictor): the checks of the former in
// their order, then the launch
static int deflate_tiles_dev(hk_ctx* ctx, int32_t dtype, const hk::DeflateTiles& r, int64_t out_capacity, int32_t stream, int32_t predictor) {
    int64_t n_tiles = 0, n_chunks = 0;
    int rc = check_deflate(ctx, dtype, r, out_capacity, &n_tiles, &n_chunks);
    if (rc || (rc = check_stream(ctx, stream))) return rc;
    if (n_chunks > 0x7FFFFFFFll) return fail(HK_ERR_ARG, "%lld chunks are more than one launch takes", (long long)n_chunks);
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[stream];
    rc = ensure_stream_ws(ctx, sl, hk::deflate_workspace_bytes(n_chunks));
    if (rc) return rc;
    HK_HIP(hk::launch_deflate_tiles(predictor, r, sl.norm_ws, sl.stream));
    return HK_OK;
}

int hk_deflate_tiles_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                         int64_t stride, int64_t band_stride, int32_t tile, void* out_dev, int64_t out_capacity,
                         int64_t* tile_offsets_dev, int64_t* tile_sizes_dev, int32_t stream) {
    const hk::DeflateTiles r = {.planes = {.src = planes_dev, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                           .band_stride = band_stride},
                                .esize = hk::dtype_size(dtype), .tile = tile, .out = static_cast<unsigned char*>(out_dev),
                                .tile_offsets = reinterpret_cast<long long*>(tile_offsets_dev),
                                .tile_sizes = reinterpret_cast<long long*>(tile_sizes_dev)};
    return deflate_tiles_dev(ctx, dtype, r, out_capacity, stream, 1);
}

int hk_deflate_tiles_pred_dev(hk_ctx* ctx, const void* planes_dev, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                              int64_t stride, int64_t band_stride, int32_t tile, void* out_dev, int64_t out_capacity,
                              int64_t* tile_offsets_dev, int64_t* tile_sizes_dev, int32_t stream, int32_t predictor) {
    const int rc = check_predictor(dtype, predictor);
    if (rc) return rc;
    const hk::DeflateTiles r = {.planes = {.src = planes_dev, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                           .band_stride = band_stride},
                                .esize = hk::dtype_size(dtype), .tile = tile, .out = static_cast<unsigned char*>(out_dev),
                                .tile_offsets = reinterpret_cast<long long*>(tile_offsets_dev),
                                .tile_sizes = reinterpret_cast<long long*>(tile_sizes_dev)};
    return deflate_tiles_dev(ctx, dtype, r, out_capacity, stream, predictor);
}

// tile rows per group of the host path: whole tile rows of ONE band of at most DEFLATE_GROUP_BYTES raw bytes (at least one tile
// row); HK_DEFLATE_GROUP_KB (read at every call) lowers the bound for tests of the group path.  Tiles are independent, so the
// grouping cannot change a byte.
constexpr size_t DEFLATE_GROUP_BYTES = 64u << 20;

// the body of hk_deflate_tiles and hk_deflate_tiles_pred (which has checked the predictor)
// (`host`: the caller's raster, streams and tables, all host memory)
static int deflate_tiles(hk_ctx* ctx, int32_t dtype, const hk::DeflateTiles& host, int64_t out_capacity, int32_t predictor) {
    int64_t n_tiles = 0, n_chunks = 0;
    int rc = check_deflate(ctx, dtype, host, out_capacity, &n_tiles, &n_chunks);
    if (rc) return rc;
    HK_ENTER(ctx);
    const int n_bands = host.planes.n_bands, height = host.planes.height, width = host.planes.width, tile = host.tile;
    const long long stride = host.planes.stride, band_stride = host.planes.band_stride;
    long long* const tile_offsets = host.tile_offsets;
    const size_t es = hk::dtype_size(dtype);
    const int64_t across = ((int64_t)width + tile - 1) / tile, down = ((int64_t)height + tile - 1) / tile;
    const size_t cap = cap_from_env("HK_DEFLATE_GROUP_KB", DEFLATE_GROUP_BYTES);
    const int64_t row_raw = across * tile * tile * (int64_t)es;   // raw bytes of one tile row
    const int64_t g_down = std::max<int64_t>(1, std::min<int64_t>(down, (int64_t)(cap / (size_t)row_raw)));
    int64_t g_tiles = 0, g_bytes = 0, g_chunks = 0;
    if ((rc = deflate_shape(dtype, 1, (int32_t)std::min<int64_t>(g_down * tile, height), width, tile, &g_tiles, &g_bytes, &g_chunks))) return rc;
    // device slab of one group: its rows (padded to ROW_ALIGN elements: 16-byte loads are legal), the chunk slots, the streams,
    // offsets and sizes
    SlabLayout L;
    const int64_t d_stride = row_align(width);
    const int64_t g_rows = std::min<int64_t>(g_down * tile, height);
    const size_t o_src = L.take((size_t)g_rows * d_stride * es);
    const size_t o_work = L.take(hk::deflate_workspace_bytes(g_chunks));
    const size_t o_out = L.take((size_t)g_bytes);
    const size_t o_off = L.take((size_t)(g_tiles + 1) * sizeof(int64_t));
    const size_t o_siz = L.take((size_t)g_tiles * sizeof(int64_t));
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    char* const base = hc.at(0);
    const char* h_src = static_cast<const char*>(host.planes.src);
    unsigned char* h_out = host.out;
    int64_t used = 0, t0 = 0;
    for (int b = 0; b < n_bands; ++b)
        for (int64_t ty = 0; ty < down; ty += g_down) {
            const int64_t r0 = ty * tile, rows = std::min<int64_t>(g_down * tile, height - r0);
            const int64_t nt = across * ((rows + tile - 1) / tile);
            if ((rc = stage_h2d(sl, base + o_src, d_stride * es, h_src + ((size_t)b * band_stride + (size_t)r0 * stride) * es,
                                stride * es, (size_t)width * es, rows)))
                return rc;
            const hk::DeflateTiles slab = {.planes = {.src = base + o_src, .n_bands = 1, .height = (int)rows, .width = width, .stride = d_stride,
                                                      .band_stride = 0},
                                           .esize = (int)es, .tile = tile, .out = hc.at<unsigned char>(o_out),
                                           .tile_offsets = hc.at<long long>(o_off), .tile_sizes = hc.at<long long>(o_siz)};
            HK_HIP(hk::launch_deflate_tiles(predictor, slab, base + o_work, sl.stream));
            // the offsets first (they say how many bytes there are), then only the compressed bytes
            if ((rc = stage_d2h(sl, tile_offsets + t0, 0, base + o_off, 0, (size_t)(nt + 1) * sizeof(int64_t), 1))) return rc;
            if ((rc = stage_d2h(sl, host.tile_sizes + t0, 0, base + o_siz, 0, (size_t)nt * sizeof(int64_t), 1))) return rc;
            if ((rc = stage_finish(sl))) return rc;
            const int64_t got = tile_offsets[t0 + nt];
            if (got < 0 || got > out_capacity - used) return fail(HK_ERR_HIP, "deflate: a group reports %lld bytes, %lld are left", (long long)got, (long long)(out_capacity - used));
            if ((rc = stage_d2h(sl, h_out + used, 0, base + o_out, 0, (size_t)got, 1))) return rc;
            if ((rc = stage_finish(sl))) return rc;
            for (int64_t k = 0; k <= nt; ++k) tile_offsets[t0 + k] += used;
            used += got, t0 += nt;
        }
    return HK_OK;
}

int hk_deflate_tiles(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width, int64_t stride,
                     int64_t band_stride, int32_t tile, void* out, int64_t out_capacity, int64_t* tile_offsets, int64_t* tile_sizes) {
    const hk::DeflateTiles r = {.planes = {.src = planes, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                           .band_stride = band_stride},
                                .esize = hk::dtype_size(dtype), .tile = tile, .out = static_cast<unsigned char*>(out),
                                .tile_offsets = reinterpret_cast<long long*>(tile_offsets),
                                .tile_sizes = reinterpret_cast<long long*>(tile_sizes)};
    return deflate_tiles(ctx, dtype, r, out_capacity, 1);
}

int hk_deflate_tiles_pred(hk_ctx* ctx, const void* planes, int32_t dtype, int32_t n_bands, int32_t height, int32_t width,
                          int64_t stride, int64_t band_stride, int32_t tile, void* out, int64_t out_capacity, int64_t* tile_offsets,
                          int64_t* tile_sizes, int32_t predictor) {
    const int rc = check_predictor(dtype, predictor);
    if (rc) return rc;
    const hk::DeflateTiles r = {.planes = {.src = planes, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                           .band_stride = band_stride},
                                .esize = hk::dtype_size(dtype), .tile = tile, .out = static_cast<unsigned char*>(out),
                                .tile_offsets = reinterpret_cast<long long*>(tile_offsets),
                                .tile_sizes = reinterpret_cast<long long*>(tile_sizes)};
    return deflate_tiles(ctx, dtype, r, out_capacity, predictor);
}

// INFLATE of a GeoTIFF image's blocks (hk_inflate.hip): see include/homonim_hk.h
struct InflateShape {
    int64_t planes, across, down, n_blocks, raw, slot;   // planes of blocks (spp if separate, else 1); full block raw bytes; its slot
    int cspp;
};

static int inflate_shape(const hk_inflate_layout* l, InflateShape* s) {
    if (!l) return fail(HK_ERR_ARG, "layout is NULL");
    if (l->sample_bytes != 1 && l->sample_bytes != 2 && l->sample_bytes != 4 && l->sample_bytes != 8)
        return fail(HK_ERR_ARG, "sample_bytes %d is not 1, 2, 4 or 8", l->sample_bytes);
    if (l->spp < 1 || l->height < 1 || l->width < 1) return fail(HK_ERR_ARG, "empty raster %d x %d x %d", l->spp, l->height, l->width);
    if (l->block_w < 1 || l->block_h < 1) return fail(HK_ERR_ARG, "empty block %d x %d", l->block_h, l->block_w);
    // (3, the floating-point predictor, is for samples of 4 and 8 bytes; those of 1 and 2 bytes have 1 and 2 alone)
    if (l->sample_bytes < 4 && l->predictor != 1 && l->predictor != 2) return fail(HK_ERR_ARG, "predictor %d is not 1 or 2", l->predictor);
    if (l->predictor < 1 || l->predictor > 3) return fail(HK_ERR_ARG, "predictor %d is not 1, 2 or 3", l->predictor);
    if ((l->tiled != 0 && l->tiled != 1) || (l->separate != 0 && l->separate != 1)) return fail(HK_ERR_ARG, "tiled and separate are 0 or 1");
    if (!l->tiled && l->block_w != l->width) return fail(HK_ERR_ARG, "a strip is as wide as the image: block_w %d, width %d", l->block_w, l->width);
    s->cspp = l->separate ? 1 : l->spp;
    s->planes = l->separate ? l->spp : 1;
    s->across = ((int64_t)l->width + l->block_w - 1) / l->block_w, s->down = ((int64_t)l->height + l->block_h - 1) / l->block_h;
    // (four factors below 2^31: the first product fits, the second is checked before it is made)
    const int64_t px = (int64_t)l->block_w * l->block_h;
    if (px > HK_INFLATE_MAX_BLOCK || px * s->cspp > HK_INFLATE_MAX_BLOCK / l->sample_bytes)
        return fail(HK_ERR_ARG, "a block of %d x %d x %d samples of %d bytes is more than %d bytes", l->block_h, l->block_w, s->cspp,
                    l->sample_bytes, HK_INFLATE_MAX_BLOCK);
    s->raw = px * s->cspp * l->sample_bytes;
    s->slot = (s->raw + 15) / 16 * 16;
    if (s->across * s->down > (1ll << 40) / s->planes || s->planes * s->across * s->down > (1ll << 62) / s->slot)
        return fail(HK_ERR_ARG, "too many blocks: %lld x %lld x %lld of %lld bytes", (long long)s->planes, (long long)s->down,
                    (long long)s->across, (long long)s->slot);
    s->n_blocks = s->planes * s->across * s->down;
    return HK_OK;
}

int hk_inflate_bound(const hk_inflate_layout* layout, int64_t* n_blocks, int64_t* raw_block_bytes, int64_t* work_bytes) {
    if (!n_blocks || !raw_block_bytes || !work_bytes) return null_arg();
    InflateShape s;
    const int rc = inflate_shape(layout, &s);
    if (rc) return rc;
    *n_blocks = s.n_blocks, *raw_block_bytes = s.raw, *work_bytes = s.n_blocks * s.slot;
    return HK_OK;
}

static const char* inflate_status_text(int st) {
    static const char* const text[] = {"ok", "the stream ends too soon", "bad zlib header", "invalid block type",
                                       "invalid stored block lengths", "invalid code lengths in a dynamic header",
                                       "invalid literal/length or distance code", "distance too far back",
                                       "the stream holds more than the block's bytes", "the stream ends before the block's bytes are there",
                                       "incorrect Adler-32 check"};
    return st >= 0 && st <= HK_INFLATE_ADLER ? text[st] : "unknown status";
}

static const char* lzw_status_text(int st) {
    static const char* const text[] = {"ok", "the stream ends too soon", "old-style (pre-6.0) LZW bit order",
                                       "the first code after a Clear is no byte", "a code beyond the table",
                                       "end of information before the block's bytes are there"};
    return st >= 0 && st <= HK_LZW_SHORT ? text[st] : "unknown status";
}

// A block image reaches the functions below as the launcher's hk::InflateArgs with the caller's part filled in by the entry: the
// streams and their table, work, status, out and the two strides.  inflate_layout_args adds the layout's part for `height` rows.
static_assert(sizeof(int) == sizeof(int32_t), "statuses are handed on as they are");
static void inflate_layout_args(hk::InflateArgs& a, const hk_inflate_layout* l, const InflateShape& s, int32_t height) {
    a.es = l->sample_bytes, a.height = height, a.width = l->width, a.bw = l->block_w, a.bh = l->block_h;
    a.tiled = l->tiled, a.separate = l->separate, a.predictor = l->predictor, a.cspp = s.cspp;
    a.across = (int)s.across, a.down = (int)(((int64_t)height + l->block_h - 1) / l->block_h), a.slot = s.slot;
}

// what every form of a block image asks of its layout, pointers and strides: the part that needs no context ...
static int check_blocks_image(const hk_inflate_layout* layout, const hk::InflateArgs& io, InflateShape* s) {
    int rc = inflate_shape(layout, s);
    if (rc) return rc;
    if (!io.streams || !io.offsets || !io.sizes || !io.out) return null_arg();
    if ((rc = check_strides(io.stride, layout->width))) return rc;
    if (io.band_stride < 0 || (layout->spp > 1 && io.band_stride < io.stride * (layout->height - 1) + layout->width))
        return fail(HK_ERR_ARG, "band_stride %lld is smaller than a plane", io.band_stride);
    return HK_OK;
}
// ... behind the context, for the forms that run on the device
static int check_inflate(hk_ctx* ctx, const hk_inflate_layout* layout, const hk::InflateArgs& io, InflateShape* s) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    return check_blocks_image(layout, io, s);
}
// the block table of the host forms (host memory): no negative offset or size
static int check_block_table(const long long* offsets, const long long* sizes, int64_t n_blocks) {
    for (int64_t b = 0; b < n_blocks; ++b)
        if (offsets[b] < 0 || sizes[b] < 0) return fail(HK_ERR_ARG, "block %lld: offset %lld, size %lld", (long long)b, offsets[b], sizes[b]);
    return HK_OK;
}

// hk_inflate_image_dev and hk_lzw_image_dev: the same call with another first kernel
static int blocks_image_dev(hk_ctx* ctx, const hk_inflate_layout* layout, hk::InflateArgs a, int32_t stream, bool lzw) {
    InflateShape s;
    int rc = check_inflate(ctx, layout, a, &s);
    if (rc) return rc;
    if (!a.work || !a.status) return null_arg();
    if ((uintptr_t)a.work % 16) return fail(HK_ERR_ARG, "work_dev is not 16-byte aligned");
    if ((uintptr_t)a.out % layout->sample_bytes) return fail(HK_ERR_ARG, "out_dev is not aligned to its samples");
    if ((rc = check_stream(ctx, stream))) return rc;
    if (s.n_blocks > 0x7FFFFFFFll) return fail(HK_ERR_ARG, "%lld blocks are more than one launch takes", (long long)s.n_blocks);
    DevEnter entered(ctx, stream);
    HK_ENTER(ctx);
    inflate_layout_args(a, layout, s, layout->height);
    HK_HIP(lzw ? hk::launch_lzw_image(a, s.n_blocks, ctx->slots[stream].stream) : hk::launch_inflate_image(a, s.n_blocks, ctx->slots[stream].stream));
    return HK_OK;
}

int hk_inflate_image_dev(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams_dev, const int64_t* offsets_dev,
                         const int64_t* sizes_dev, void* work_dev, void* out_dev, int64_t stride, int64_t band_stride,
                         int32_t* status_dev, int32_t stream) {
    return blocks_image_dev(ctx, layout, {.streams = streams_dev, .offsets = reinterpret_cast<const long long*>(offsets_dev),
                                          .sizes = reinterpret_cast<const long long*>(sizes_dev), .work = static_cast<unsigned char*>(work_dev),
                                          .status = status_dev, .out = out_dev, .stride = stride, .band_stride = band_stride}, stream, false);
}

int hk_lzw_image_dev(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams_dev, const int64_t* offsets_dev,
                     const int64_t* sizes_dev, void* work_dev, void* out_dev, int64_t stride, int64_t band_stride,
                     int32_t* status_dev, int32_t stream) {
    return blocks_image_dev(ctx, layout, {.streams = streams_dev, .offsets = reinterpret_cast<const long long*>(offsets_dev),
                                          .sizes = reinterpret_cast<const long long*>(sizes_dev), .work = static_cast<unsigned char*>(work_dev),
                                          .status = status_dev, .out = out_dev, .stride = stride, .band_stride = band_stride}, stream, true);
}

// block rows per group of the host path: whole block rows of ALL planes, at most INFLATE_GROUP_BYTES of raw bytes (at least one
// block row); HK_INFLATE_GROUP_KB (read at every call) lowers the bound for tests of the group path.  Blocks are independent, so
// the grouping cannot change a byte.  Per group and plane the compressed bytes travel as ONE span of the caller's buffer, from the
// first byte of the group's first stream to the last byte of its last one (a TIFF writer lays the blocks of a plane down in order).
constexpr size_t INFLATE_GROUP_BYTES = 64u << 20;

// (hk_inflate_image and hk_lzw_image: the same call with another first kernel)
// `host`: the caller's streams, table, raster and statuses (nullable), all host memory
static int blocks_image(hk_ctx* ctx, const hk_inflate_layout* layout, const hk::InflateArgs& host, bool lzw) {
    InflateShape s;
    int rc = check_inflate(ctx, layout, host, &s);
    if (rc || (rc = check_block_table(host.offsets, host.sizes, s.n_blocks))) return rc;
    HK_ENTER(ctx);
    const long long *const offsets = host.offsets, *const sizes = host.sizes, stride = host.stride, band_stride = host.band_stride;
    int* const status = host.status;
    const size_t es = (size_t)layout->sample_bytes;
    const int64_t bh = layout->block_h, per = s.across * s.down;
    const size_t cap = cap_from_env("HK_INFLATE_GROUP_KB", INFLATE_GROUP_BYTES);
    const int64_t row_raw = s.planes * s.across * s.slot;   // slots of one block row
    const int64_t g_down = std::max<int64_t>(1, std::min<int64_t>(s.down, (int64_t)(cap / (size_t)row_raw)));
    const int64_t g_blocks = s.planes * g_down * s.across;
    if (g_blocks > 0x7FFFFFFFll) return fail(HK_ERR_ARG, "%lld blocks are more than one launch takes", (long long)g_blocks);
    // the spans of every group and plane: where they start in the caller's buffer and how long they are; the largest sum over a group
    struct Span { long long lo, hi; };
    auto span_of = [&](int64_t plane, int64_t by0, int64_t by1) {
        Span sp{INT64_MAX, 0};
        for (int64_t b = plane * per + by0 * s.across; b < plane * per + by1 * s.across; ++b)
            if (sizes[b] > 0) sp.lo = std::min(sp.lo, offsets[b]), sp.hi = std::max(sp.hi, offsets[b] + sizes[b]);
        if (sp.lo > sp.hi) sp.lo = sp.hi = 0;
        sp.lo &= ~(int64_t)15;   // (the device copy keeps the streams' places within their 16-byte groups)
        return sp;
    };
    size_t in_bytes = 0;
    for (int64_t by0 = 0; by0 < s.down; by0 += g_down) {
        size_t sum = 0;
        for (int64_t p = 0; p < s.planes; ++p) {
            const Span sp = span_of(p, by0, std::min(s.down, by0 + g_down));
            sum += ((size_t)(sp.hi - sp.lo) + 255) / 256 * 256;
        }
        in_bytes = std::max(in_bytes, sum);
    }
    // device slab of one group: the compressed spans, offsets and sizes, the statuses, the slots, the group's rows of every band
    // (padded to ROW_ALIGN elements: 16-byte stores are legal)
    SlabLayout L;
    const int64_t d_stride = row_align(layout->width);
    const int64_t g_rows = std::min<int64_t>(g_down * bh, layout->height);
    const size_t o_in = L.take(in_bytes);
    const size_t o_off = L.take((size_t)g_blocks * sizeof(int64_t));
    const size_t o_siz = L.take((size_t)g_blocks * sizeof(int64_t));
    const size_t o_st = L.take((size_t)g_blocks * sizeof(int32_t));
    const size_t o_work = L.take((size_t)g_blocks * (size_t)s.slot);
    const size_t o_out = L.take((size_t)layout->spp * g_rows * d_stride * es);
    HostCall hc(ctx, L.total);
    if (hc.rc) return hc.rc;
    Slot& sl = hc.sl;
    char* const base = hc.at(0);
    const char* h_in = static_cast<const char*>(host.streams);
    char* h_out = static_cast<char*>(host.out);
    std::vector<int64_t> g_off((size_t)g_blocks), g_siz((size_t)g_blocks);
    std::vector<int32_t> g_st((size_t)g_blocks);
    int64_t first_bad = -1;
    int32_t first_status = 0;
    for (int64_t by0 = 0; by0 < s.down; by0 += g_down) {
        const int64_t by1 = std::min(s.down, by0 + g_down), n_down = by1 - by0, nb = s.planes * n_down * s.across;
        const int64_t r0 = by0 * bh, rows = std::min<int64_t>(n_down * bh, layout->height - r0);
        size_t at = 0;
        for (int64_t p = 0; p < s.planes; ++p) {
            const Span sp = span_of(p, by0, by1);
            if ((rc = stage_h2d(sl, base + o_in + at, 0, h_in + sp.lo, 0, (size_t)(sp.hi - sp.lo), 1))) return rc;
            for (int64_t k = 0; k < n_down * s.across; ++k) {
                const int64_t b = p * per + by0 * s.across + k;
                g_off[(size_t)(p * n_down * s.across + k)] = sizes[b] > 0 ? (int64_t)at + offsets[b] - sp.lo : 0;
                g_siz[(size_t)(p * n_down * s.across + k)] = sizes[b];
            }
            at += ((size_t)(sp.hi - sp.lo) + 255) / 256 * 256;
        }
        if ((rc = stage_h2d(sl, base + o_off, 0, g_off.data(), 0, (size_t)nb * sizeof(int64_t), 1))) return rc;
        if ((rc = stage_h2d(sl, base + o_siz, 0, g_siz.data(), 0, (size_t)nb * sizeof(int64_t), 1))) return rc;
        hk::InflateArgs a = {.streams = base + o_in, .offsets = hc.at<long long>(o_off), .sizes = hc.at<long long>(o_siz),
                             .work = hc.at<unsigned char>(o_work), .status = hc.at<int>(o_st), .out = base + o_out, .stride = d_stride,
                             .band_stride = rows * d_stride};
        inflate_layout_args(a, layout, s, (int32_t)rows);
        HK_HIP(lzw ? hk::launch_lzw_image(a, nb, sl.stream) : hk::launch_inflate_image(a, nb, sl.stream));
        if ((rc = stage_d2h(sl, g_st.data(), 0, base + o_st, 0, (size_t)nb * sizeof(int32_t), 1))) return rc;
        for (int c = 0; c < layout->spp; ++c)
            if ((rc = stage_d2h(sl, h_out + ((size_t)c * band_stride + (size_t)r0 * stride) * es, stride * es,
                                base + o_out + (size_t)c * rows * d_stride * es, d_stride * es, (size_t)layout->width * es, rows)))
                return rc;
        if ((rc = stage_finish(sl))) return rc;
        for (int64_t p = 0; p < s.planes; ++p)
            for (int64_t k = 0; k < n_down * s.across; ++k) {
                const int64_t b = p * per + by0 * s.across + k;
                const int32_t st = g_st[(size_t)(p * n_down * s.across + k)];
                if (status) status[b] = st;
                if (st && (first_bad < 0 || b < first_bad)) first_bad = b, first_status = st;
            }
    }
    if (first_bad >= 0)
        return fail(HK_ERR_ARG, "%s: block %lld is refused: %s (status %d)", lzw ? "lzw" : "inflate", (long long)first_bad,
                    lzw ? lzw_status_text(first_status) : inflate_status_text(first_status), first_status);
    return HK_OK;
}

int hk_inflate_image(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams, const int64_t* offsets, const int64_t* sizes,
                     void* out, int64_t stride, int64_t band_stride, int32_t* status) {
    return blocks_image(ctx, layout, {.streams = streams, .offsets = reinterpret_cast<const long long*>(offsets),
                                      .sizes = reinterpret_cast<const long long*>(sizes), .status = status, .out = out, .stride = stride,
                                      .band_stride = band_stride}, false);
}

int hk_lzw_image(hk_ctx* ctx, const hk_inflate_layout* layout, const void* streams, const int64_t* offsets, const int64_t* sizes,
                 void* out, int64_t stride, int64_t band_stride, int32_t* status) {
    return blocks_image(ctx, layout, {.streams = streams, .offsets = reinterpret_cast<const long long*>(offsets),
                                      .sizes = reinterpret_cast<const long long*>(sizes), .status = status, .out = out, .stride = stride,
                                      .band_stride = band_stride}, true);
}

// the same image on the calling thread (hk_lzw_host.hip): no context, no device
int hk_lzw_image_host(const hk_inflate_layout* layout, const void* streams, const int64_t* offsets, const int64_t* sizes, void* out,
                      int64_t stride, int64_t band_stride, int32_t* status) {
    InflateShape s;
    hk::InflateArgs a = {.streams = streams, .offsets = reinterpret_cast<const long long*>(offsets),
                         .sizes = reinterpret_cast<const long long*>(sizes), .status = status, .out = out, .stride = stride,
                         .band_stride = band_stride};
    int rc = check_blocks_image(layout, a, &s);
    if (rc) return rc;
    if ((uintptr_t)out % layout->sample_bytes) return fail(HK_ERR_ARG, "out is not aligned to its samples");
    if ((rc = check_block_table(a.offsets, a.sizes, s.n_blocks))) return rc;
    std::vector<uint64_t> slot((size_t)s.slot / 8 + 2);   // (8-byte aligned for every sample size; the slot is a multiple of 16)
    inflate_layout_args(a, layout, s, layout->height);
    a.work = reinterpret_cast<unsigned char*>(slot.data());
    int first_status = 0;
    const long long first_bad = hk::lzw_image_host(a, s.n_blocks, &first_status);
    if (first_bad >= 0)
        return fail(HK_ERR_ARG, "lzw: block %lld is refused: %s (status %d)", first_bad, lzw_status_text(first_status), first_status);
    return HK_OK;
}

int hk_block_norm_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, double* norm_dev) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_job(ctx, job);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (!norm_dev) return fail(HK_ERR_ARG, "norm_dev is NULL");
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    rc = ensure_stream_ws(ctx, sl, hk::norm_workspace_bytes(job->n_bands, job->height, job->width));
    if (rc) return rc;
    const hk::NormArgs na = norm_args(desc, job->src, job->ref, job->height, job->width, job->stride, job->band_stride, job->n_bands);
    HK_HIP(hk::launch_block_norm(na, sl.norm_ws, norm_dev, sl.stream));
    return HK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched device entry points: many jobs, one launch per kernel stage, all on jobs[0].stream.

// Upload `bytes` of table data to a device buffer of the slot's ring; *dev_out is valid for the kernels queued next on the
// slot's stream (and until the ring comes round: TBL_RING uploads later, which the stream has ordered behind them).
static int upload_table(hk_ctx* ctx, Slot& sl, const void* data, size_t bytes, void** dev_out) {
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int i = sl.tbl_next;
    sl.tbl_next = (sl.tbl_next + 1) % Slot::TBL_RING;
    if (!sl.tbl_ev[i]) HK_HIP(hipEventCreateWithFlags(&sl.tbl_ev[i], hipEventDisableTiming));
    else HK_HIP(hipEventSynchronize(sl.tbl_ev[i]));  // the upload that last used this entry's host buffer has been made
    if (sl.tbl_bytes[i] < bytes) {
        if (sl.tbl_dev[i]) {
            HK_HIP(hipStreamSynchronize(sl.stream));  // kernels may still read the old device buffer
            HK_HIP(dev_free(sl.tbl_dev[i]));
            HK_HIP(hipHostFree(sl.tbl_host[i]));
        }
        sl.tbl_dev[i] = sl.tbl_host[i] = nullptr, sl.tbl_bytes[i] = 0;
        const size_t cap = (bytes + 4095) / 4096 * 4096;
        if (dev_malloc(&sl.tbl_dev[i], cap) != hipSuccess) return fail(HK_ERR_NOMEM, "hipMalloc(%zu) failed", cap);
        if (hipHostMalloc(&sl.tbl_host[i], cap, hipHostMallocDefault) != hipSuccess) {
            (void)dev_free(sl.tbl_dev[i]);
            sl.tbl_dev[i] = nullptr;
            return fail(HK_ERR_NOMEM, "hipHostMalloc(%zu) failed", cap);
        }
        sl.tbl_bytes[i] = cap;
    }
    memcpy(sl.tbl_host[i], data, bytes);
    HK_HIP(hipMemcpyAsync(sl.tbl_dev[i], sl.tbl_host[i], bytes, hipMemcpyHostToDevice, sl.stream));
    HK_HIP(hipEventRecord(sl.tbl_ev[i], sl.stream));
    *dev_out = sl.tbl_dev[i];
    return HK_OK;
}

static int check_batch(hk_ctx* ctx, const hk_dev_job* jobs, int32_t n_jobs) {
    if (!ctx || !jobs) return fail(HK_ERR_ARG, "NULL argument");
    if (n_jobs < 1 || n_jobs > 65536) return fail(HK_ERR_ARG, "n_jobs %d outside 1..65536", n_jobs);
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (jobs[j].stream != jobs[0].stream) return fail(HK_ERR_ARG, "the jobs of a batch share one stream (job %d differs)", j);
        const int rc = check_job(ctx, &jobs[j]);
        if (rc) return rc;
    }
    return HK_OK;
}

int hk_block_norm_batch_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* jobs, int32_t n_jobs, double* norm_dev) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_batch(ctx, jobs, n_jobs);
    if (rc) return rc;
    DevEnter entered(ctx, jobs[0].stream);
    if (!norm_dev) return fail(HK_ERR_ARG, "norm_dev is NULL");
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[jobs[0].stream];
    std::vector<hk::NormPlane> planes;
    int max_h = 0, max_w = 0, max_waves = 0;
    long long max_px = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        const hk_dev_job& job = jobs[j];
        for (int32_t b = 0; b < job.n_bands; ++b) {
            hk::NormPlane pl;
            pl.src = job.src + (long long)b * job.band_stride, pl.ref = job.ref + (long long)b * job.band_stride;
            pl.stride = job.stride, pl.height = job.height, pl.width = job.width;
            planes.push_back(pl);
        }
        // the plane with the most pixels sizes the compaction buffers of every plane, the one with the most 1 KB chunks the grid
        // of the streaming pass (not the same plane in general: 1090 x 1025 has fewer pixels but more chunks than 1100 x 1024)
        if ((long long)job.height * job.width > max_px) max_px = (long long)job.height * job.width, max_h = job.height, max_w = job.width;
        max_waves = std::max(max_waves, hk::norm_pass_waves(job.height, job.width));
    }
    // grid.y of the select passes = 2 x planes
    if (planes.size() > 32767) return fail(HK_ERR_ARG, "a statistics batch holds at most 32767 planes (jobs x bands)");
    rc = ensure_stream_ws(ctx, sl, hk::norm_workspace_bytes((int)planes.size(), max_h, max_w));
    if (rc) return rc;
    void* tbl = nullptr;
    rc = upload_table(ctx, sl, planes.data(), planes.size() * sizeof(hk::NormPlane), &tbl);
    if (rc) return rc;
    hk::NormArgs na = norm_args(desc, nullptr, nullptr, max_h, max_w, 0, 0, (int)planes.size());
    na.planes = static_cast<const hk::NormPlane*>(tbl);
    na.grid_waves = max_waves;
    HK_HIP(hk::launch_block_norm(na, sl.norm_ws, norm_dev, sl.stream));
    return HK_OK;
}

int hk_fit_apply_batch_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* jobs, int32_t n_jobs) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_batch(ctx, jobs, n_jobs);
    if (rc) return rc;
    DevEnter entered(ctx, jobs[0].stream);
    for (int32_t j = 1; j < n_jobs; ++j) {
        const hk_dev_job* job = &jobs[j];
        // what selects the kernel build must not differ inside a launch (the contract holds for every model)
        if ((!job->gain) != (!jobs[0].gain) || (!job->offset) != (!jobs[0].offset) || (!job->r2) != (!jobs[0].r2) ||
            (!job->corr) != (!jobs[0].corr) || (!job->fail_count) != (!jobs[0].fail_count) || (!job->scratch) != (!jobs[0].scratch))
            return fail(HK_ERR_ARG, "the jobs of a batch ask for the same set of outputs (job %d differs from job 0)", j);
    }
    if (!hk::fit_batch_build(desc->model, needs_r2(desc))) {
        // builds without the job-table look-up (hk_kernels.h fit_batch_build): one launch per job, in order, same results
        for (int32_t j = 0; j < n_jobs; ++j) {
            rc = hk_fit_apply_dev(ctx, desc, &jobs[j]);
            if (rc) return rc;
        }
        return HK_OK;
    }
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[jobs[0].stream];
    std::vector<hk::FitArgs> args((size_t)n_jobs);
    std::vector<long long> first((size_t)n_jobs + 1, 0);  // first unit of each job in the launch
    bool any_explicit = false;
    for (int32_t j = 0; j < n_jobs; ++j) {
        if (desc->model == HK_MODEL_GAIN_BLK_OFFSET && !jobs[j].norm) return fail(HK_ERR_ARG, "gain-blk-offset needs job->norm (job %d)", j);
        hk::FitArgs& a = args[(size_t)j];
        if ((rc = job_fit_args(a, ctx, desc, jobs[j]))) return rc;
        any_explicit |= jobs[j].seg_rows > 0 || a.seg_rows_pref > 0;
        first[(size_t)j + 1] = first[(size_t)j] + (long long)a.n_strips * a.n_segs * a.n_bands;
    }
    // seg_policy() applied to the LAUNCH: the jobs run in order, so the jobs whose units make up its tail get short segments
    // (they level the end of the launch) and all earlier ones long segments.  Results do not depend on the segment height
    // (exact running sums).
    const SegPolicy seg = seg_policy(desc->kh, ctx->launch);
    const long long units = first[(size_t)n_jobs];
    if (!any_explicit && units >= seg.two_size_from) {
        const long long tail_from = units - (long long)seg.tail_waves;
        for (int32_t j = 0; j < n_jobs; ++j) {
            const int rows = first[(size_t)j + 1] <= tail_from ? seg.big : seg.tail;
            if (rows > 0) fill_grid(args[(size_t)j], rows, ctx->launch);
        }
    }
    // (only models without the r2 mask have builds with the job-table look-up: no certificate, no in-painting inputs here)
    const int wpb = hk::WPB_MEM;
    std::vector<hk::FitJob> table((size_t)n_jobs);
    long long groups[2] = {0, 0}, total_px = 0;
    for (int32_t j = 0; j < n_jobs; ++j) {
        const hk::FitArgs& a = args[(size_t)j];
        hk::FitJob& e = table[(size_t)j];
        hk::fit_job_of(e, a);
        e.first_group[0] = (int)groups[0], e.first_group[1] = (int)groups[1];
        groups[0] += (long long)a.n_strips * a.n_segs * a.n_bands;
        groups[1] += (long long)((a.n_strips + wpb - 1) / wpb) * a.n_segs * a.n_bands;
        total_px += (long long)a.height * a.width * a.n_bands;
        if (groups[0] > 0x7fffff00ll) return fail(HK_ERR_ARG, "the batch has too many wave units for one launch");
    }
    hk::FitArgs a0 = args[0];  // the launch's argument block: everything the jobs share, and job 0's own fields (which the table overrides)
    a0.cert_only = 0;
    a0.n_jobs = n_jobs;
    a0.batch_groups[0] = (int)groups[0], a0.batch_groups[1] = (int)groups[1];
    if (lds_pad_by_size(desc, ctx->launch)) a0.lds_pad = lds_pad_of(total_px);  // by the size of the whole launch
    void* tbl = nullptr;
    rc = upload_table(ctx, sl, table.data(), table.size() * sizeof(hk::FitJob), &tbl);
    if (rc) return rc;
    a0.jobs = static_cast<const hk::FitJob*>(tbl);
    HK_HIP(hk::launch_fit_apply(a0, desc->model, needs_r2(desc), sl.stream));
    return HK_OK;
}

int hk_fail_counts_batch_async(hk_ctx* ctx, const hk_dev_job* jobs, int32_t n_jobs, uint64_t* host_counts, hk_event* ready) {
    int rc = check_batch(ctx, jobs, n_jobs);
    if (rc) return rc;
    DevEnter entered(ctx, jobs[0].stream);
    if (!host_counts || !ready) return fail(HK_ERR_ARG, "NULL argument");
    for (int32_t j = 0; j < n_jobs; ++j)
        if (!jobs[j].fail_count) return fail(HK_ERR_ARG, "job %d has no fail_count", j);
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[jobs[0].stream];
    {
        size_t n_all = 0;
        for (int32_t j = 0; j < n_jobs; ++j) n_all += (size_t)jobs[j].n_bands;
        if (!host_is_pinned(host_counts, n_all * sizeof(uint64_t)))
            return fail(HK_ERR_ARG, "host_counts must be page-locked memory (hk_host_alloc / hk_host_register)");
    }
    // one copy + one clearing per run of jobs whose counters lie back to back in device memory (a caller that allocates the
    // counters of a batch as one array gets exactly one of each)
    size_t done = 0;  // counters copied so far = offset into host_counts
    for (int32_t j = 0; j < n_jobs;) {
        uint64_t* const first = jobs[j].fail_count;
        size_t n = (size_t)jobs[j].n_bands;
        int32_t k = j + 1;
        while (k < n_jobs && jobs[k].fail_count == first + n) n += (size_t)jobs[k].n_bands, ++k;
        HK_HIP(hipMemcpyAsync(host_counts + done, first, n * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.stream));
        HK_HIP(hipMemsetAsync(first, 0, n * sizeof(uint64_t), sl.stream));
        done += n, j = k;
    }
    HK_HIP(hipEventRecord(ready->ev, sl.stream));
    return HK_OK;
}

uint64_t hk_block_norm_split_exchange_doubles(int32_t n_bands) {
    return n_bands > 0 ? (uint64_t)hk::norm_split_exchange_doubles(n_bands) : 0;
}

int hk_block_norm_split_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, int32_t phase, int32_t world_size,
                            double* xchg_dev, double* norm_dev) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_job(ctx, job, /*allow_no_rows=*/true);  // a rank without rows of the block takes part with zeros
    if (rc) return rc;
    if (!xchg_dev || !norm_dev) return fail(HK_ERR_ARG, "xchg_dev / norm_dev is NULL");
    if (phase < 0 || phase > 5) return fail(HK_ERR_ARG, "phase %d outside 0..5", phase);
    if (world_size < 1) return fail(HK_ERR_ARG, "world_size < 1");
    DevEnter entered(ctx, job->stream);
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    // the phases of one block share the stream's workspace: phase 0 sizes it, the others find it as it was left
    rc = ensure_stream_ws(ctx, sl, hk::norm_workspace_bytes(job->n_bands, job->height > 0 ? job->height : 1, job->width));
    if (rc) return rc;
    const hk::NormArgs na = norm_args(desc, job->src, job->ref, job->height, job->width, job->stride, job->band_stride, job->n_bands);
    HK_HIP(hk::launch_block_norm_split(na, sl.norm_ws, xchg_dev, phase, norm_dev, sl.stream));
    return HK_OK;
}

int hk_comm_unique_id(uint8_t id[HK_COMM_ID_BYTES]) {
    static_assert(HK_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "hk_comm id = ncclUniqueId");
    if (!id) return fail(HK_ERR_ARG, "id is NULL");
    if (!rccl().ok) return fail(HK_ERR_UNSUPPORTED, "librccl could not be opened");
    ncclUniqueId u;
    HK_RCCL(rccl().GetUniqueId(&u));
    memcpy(id, u.internal, HK_COMM_ID_BYTES);
    return HK_OK;
}

int hk_comm_init(hk_ctx* ctx, const uint8_t id[HK_COMM_ID_BYTES], int32_t rank, int32_t world_size) {
    if (!ctx || !id) return fail(HK_ERR_ARG, "NULL argument");
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(HK_ERR_ARG, "rank %d outside a group of %d", rank, world_size);
    if (!rccl().ok) return fail(HK_ERR_UNSUPPORTED, "librccl could not be opened");
    std::lock_guard<std::mutex> lk(ctx->comm_mu);
    if (ctx->comm) return fail(HK_ERR_ARG, "the context has a communicator already (hk_comm_destroy it first)");
    HK_ENTER(ctx);
    ncclUniqueId u;
    memcpy(u.internal, id, HK_COMM_ID_BYTES);
    ncclComm_t c = nullptr;
    HK_RCCL(rccl().CommInitRank(&c, world_size, u, rank));  // collective: returns once every rank has joined
    ctx->comm = c, ctx->comm_rank = rank, ctx->comm_world = world_size;
    return HK_OK;
}

int hk_comm_destroy(hk_ctx* ctx) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    std::lock_guard<std::mutex> lk(ctx->comm_mu);
    if (!ctx->comm) return HK_OK;
    HK_ENTER(ctx);
    HK_HIP(hipDeviceSynchronize());
    HK_RCCL(rccl().CommDestroy(ctx->comm));
    ctx->comm = nullptr, ctx->comm_rank = ctx->comm_world = 0;
    return HK_OK;
}

int hk_comm_info(hk_ctx* ctx, int32_t* rank, int32_t* world_size) {
    if (!ctx || !rank || !world_size) return fail(HK_ERR_ARG, "NULL argument");
    std::lock_guard<std::mutex> lk(ctx->comm_mu);
    *rank = ctx->comm ? ctx->comm_rank : -1;
    *world_size = ctx->comm ? ctx->comm_world : 0;
    return HK_OK;
}

int hk_comm_allreduce_f64_dev(hk_ctx* ctx, double* buf_dev, uint64_t count, int32_t stream) {
    if (!ctx || !buf_dev) return fail(HK_ERR_ARG, "NULL argument");
    if (const int bad = check_stream(ctx, stream)) return bad;
    std::lock_guard<std::mutex> lk(ctx->comm_mu);
    if (!ctx->comm) return fail(HK_ERR_ARG, "the context has no communicator (hk_comm_init)");
    HK_ENTER(ctx);
    HK_RCCL(rccl().AllReduce(buf_dev, buf_dev, count, ncclDouble, ncclSum, ctx->comm, ctx->slots[stream].stream));
    return HK_OK;
}

int hk_block_norm_split_comm_dev(hk_ctx* ctx, const hk_fit_desc* desc, const hk_dev_job* job, double* norm_dev) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    rc = check_job(ctx, job, /*allow_no_rows=*/true);
    if (rc) return rc;
    DevEnter entered(ctx, job->stream);
    if (!norm_dev) return fail(HK_ERR_ARG, "norm_dev is NULL");
    std::lock_guard<std::mutex> lk(ctx->comm_mu);  // one collective sequence at a time per communicator, every rank alike
    if (!ctx->comm) return fail(HK_ERR_ARG, "the context has no communicator (hk_comm_init)");
    HK_ENTER(ctx);
    Slot& sl = ctx->slots[job->stream];
    rc = ensure_stream_ws(ctx, sl, hk::norm_workspace_bytes(job->n_bands, job->height > 0 ? job->height : 1, job->width));
    if (rc) return rc;
    const size_t n = hk::norm_split_exchange_doubles(job->n_bands);
    rc = grow_slot_buf(sl, sl.comm_xchg, sl.comm_xchg_bytes, n * sizeof(double));
    if (rc) return rc;
    const hk::NormArgs na = norm_args(desc, job->src, job->ref, job->height, job->width, job->stride, job->band_stride, job->n_bands);
    // six phases on the slab, five all-reduces between them, all queued on the job's stream: no host synchronisation
    for (int phase = 0; phase < 6; ++phase) {
        HK_HIP(hk::launch_block_norm_split(na, sl.norm_ws, sl.comm_xchg, phase, norm_dev, sl.stream));
        if (phase < 5)
            HK_RCCL(rccl().AllReduce(sl.comm_xchg, sl.comm_xchg, n, ncclDouble, ncclSum, ctx->comm, sl.stream));
    }
    return HK_OK;
}

int hk_synth_fill_dev(hk_ctx* ctx, float* src, float* ref, int32_t n_bands, int32_t height, int32_t width,
                      int64_t stride, int64_t band_stride, uint64_t seed, int32_t nodata_variant, int32_t stream) {
    if (!ctx || !src || !ref) return fail(HK_ERR_ARG, "NULL argument");
    if (const int bad = check_stream(ctx, stream)) return bad;
    HK_ENTER(ctx);
    HK_HIP(hk::launch_synth_fill({.src = src, .ref = ref, .n_bands = n_bands, .height = height, .width = width, .stride = stride,
                                  .band_stride = band_stride, .seed = seed, .nodata_variant = nodata_variant},
                                 ctx->slots[stream].stream));
    return HK_OK;
}

int hk_stream_probe_dev(hk_ctx* ctx, const void* a, const void* b, void* out, size_t n_bytes, int32_t stream) {
    if (!ctx || !a || !b || !out) return fail(HK_ERR_ARG, "NULL argument");
    if (n_bytes % 16) return fail(HK_ERR_ARG, "n_bytes must be a multiple of 16");
    if (const int bad = check_stream(ctx, stream)) return bad;
    HK_ENTER(ctx);
    HK_HIP(hk::launch_stream_probe(a, b, out, n_bytes, ctx->slots[stream].stream));
    return HK_OK;
}

int hk_debug_checksum_dev(hk_ctx* ctx, const float* plane, int64_t stride, int32_t height, int32_t width, int32_t stream,
                          uint64_t* sum_out) {
    if (!ctx || !plane || !sum_out) return fail(HK_ERR_ARG, "NULL argument");
    if (height < 1 || width < 1 || stride < width) return fail(HK_ERR_ARG, "bad window %d x %d, stride %lld", height, width, (long long)stride);
    if (const int bad = check_stream(ctx, stream)) return bad;
    HK_ENTER(ctx);
    DevEnter enter(ctx, stream);
    Slot& sl = ctx->slots[stream];
    // the slot's pinned counter word doubles as the device-visible accumulator's landing place
    unsigned long long* d_acc = nullptr;
    if (dev_malloc(reinterpret_cast<void**>(&d_acc), sizeof(unsigned long long)) != hipSuccess) return fail(HK_ERR_NOMEM, "hipMalloc(8) failed");
    hipError_t e = hipMemsetAsync(d_acc, 0, sizeof(unsigned long long), sl.stream);
    if (e == hipSuccess) e = hk::launch_checksum(plane, stride, height, width, d_acc, sl.stream);
    unsigned long long host = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(sl.fail_host, d_acc, sizeof(host), hipMemcpyDeviceToHost, sl.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(sl.stream);
    if (e == hipSuccess) host = *sl.fail_host;
    (void)dev_free(d_acc);
    if (e != hipSuccess) return fail(HK_ERR_HIP, "checksum: %s", hipGetErrorString(e));
    *sum_out = host;
    return HK_OK;
}

int hk_debug_inpaint_plane_dev(hk_ctx* ctx, float* plane_dev, const uint8_t* flags_dev, const float* gain_dev, const float* r2_dev,
                               float thresh, int32_t height, int32_t width, int64_t stride, int32_t mode, int32_t stream) {
    if (!ctx || !plane_dev) return fail(HK_ERR_ARG, "NULL argument");
    if (const int bad = check_stream(ctx, stream)) return bad;
    if (mode < 0 || mode > 3) return fail(HK_ERR_ARG, "mode %d: 0 (the library's choice), 1 / 2 (packed search by rows / columns), 3 (general search only)", mode);
    // the bit planes' launches take one grid row per 64 raster rows
    if (height < 1 || width < 1 || height > 65535 * 64) return fail(HK_ERR_ARG, "bad shape %d x %d", height, width);
    // rows are read as 4-byte flag groups, stored as 8-byte table pairs and staged as 16-byte table quads
    if (stride < width || stride % 4 != 0) return fail(HK_ERR_ARG, "stride %lld: at least the width (%d) and a multiple of 4", (long long)stride, width);
    // (launch_inpaint_offsets leaves the packed search out at such a stride: modes 1 and 2 would not run what they name)
    if ((mode == 1 || mode == 2) && stride >= (1ll << 23))
        return fail(HK_ERR_ARG, "mode %d: the packed search takes strides below 2^23 only (stride %lld)", mode, (long long)stride);
    if (flags_dev ? (gain_dev || r2_dev) : (!gain_dev || !r2_dev))
        return fail(HK_ERR_ARG, "give either flags_dev or both of gain_dev and r2_dev");
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; };
    if (misaligned(plane_dev) || misaligned(flags_dev) || misaligned(gain_dev) || misaligned(r2_dev))
        return fail(HK_ERR_ARG, "device planes must be 4-byte aligned (the flag plane too: it is read four columns at a time)");
    HK_ENTER(ctx);
    DevEnter entered(ctx, stream);
    Slot& sl = ctx->slots[stream];
    InpaintScratch s;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);  // the slot's scratch may be (re)allocated
        const int rc = inpaint_scratch(sl, height, stride, s);
        if (rc) return rc;
    }
    unsigned long long n_targets = 0;  // mode 1: unknown -> row order
    if (mode == 2) n_targets = (unsigned long long)height * (unsigned long long)width;  // every pixel failing -> column order
    if (mode == 0) {  // as inpaint_band is told by the pass that counted: the number of pixels that are not sources
        const size_t n = (size_t)height * (size_t)stride;
        std::vector<uint8_t> hf;
        std::vector<float> hg, hr;
        try {
            hf.resize(flags_dev ? n : 0), hg.resize(flags_dev ? 0 : n), hr.resize(flags_dev ? 0 : n);
        } catch (...) {
            return fail(HK_ERR_NOMEM, "out of host memory (counting the targets of %d x %lld pixels)", height, (long long)stride);
        }
        HK_HIP(hipStreamSynchronize(sl.stream));
        if (flags_dev) {
            HK_HIP(hipMemcpy(hf.data(), flags_dev, n, hipMemcpyDeviceToHost));
        } else {
            HK_HIP(hipMemcpy(hg.data(), gain_dev, n * sizeof(float), hipMemcpyDeviceToHost));
            HK_HIP(hipMemcpy(hr.data(), r2_dev, n * sizeof(float), hipMemcpyDeviceToHost));
        }
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) {
                const size_t i = (size_t)y * (size_t)stride + x;
                n_targets += flags_dev ? hf[i] == 0 : !((hr[i] > thresh) && (hg[i] > 0.f));
            }
    }
    hk::InpaintArgs ia;
    ia.offset = plane_dev, ia.stride = stride, ia.height = height, ia.width = width;
    ia.flag_ready = flags_dev, ia.gain = gain_dev, ia.r2 = r2_dev, ia.thresh = thresh;
    ia.n_targets = n_targets, ia.packed_search = mode != 3;
    HK_HIP(hk::launch_inpaint_offsets(ia, s.ws, sl.stream));
    HK_HIP(hipStreamSynchronize(sl.stream));
    return HK_OK;
}

int hk_debug_cast_plane_dev(hk_ctx* ctx, int32_t to_typed, int32_t dtype, const void* src_dev, int64_t src_stride, void* dst_dev,
                            int64_t dst_stride, int32_t height, int32_t width, int32_t has_nodata, double nodata, int32_t stream) {
    if (!ctx || !src_dev || !dst_dev) return fail(HK_ERR_ARG, "NULL argument");
    if (const int bad = check_stream(ctx, stream)) return bad;
    if (to_typed != 0 && to_typed != 1) return fail(HK_ERR_ARG, "to_typed %d: 0 (cast_in) or 1 (cast_out)", to_typed);
    const size_t es = hk::dtype_size(dtype);
    if (!es) return fail(HK_ERR_ARG, "unknown dtype %d", dtype);
    if (!to_typed && dtype == HK_DTYPE_F32) return fail(HK_ERR_ARG, "float32 has no input conversion");
    if (height < 1 || width < 1) return fail(HK_ERR_ARG, "bad shape %d x %d", height, width);
    // a lane takes four columns at once: the float32 side as one 16-byte access, the typed side sample by sample
    for (const int64_t s : {src_stride, dst_stride})
        if (s < width || s % 4 != 0) return fail(HK_ERR_ARG, "stride %lld: at least the width (%d) and a multiple of 4", (long long)s, width);
    const void *f32_plane = to_typed ? src_dev : dst_dev, *typed_plane = to_typed ? static_cast<const void*>(dst_dev) : src_dev;
    if ((reinterpret_cast<uintptr_t>(f32_plane) & 15u) != 0 || reinterpret_cast<uintptr_t>(typed_plane) % es != 0)
        return fail(HK_ERR_ARG, "the float32 plane must be 16-byte aligned, the typed plane aligned to its sample size");
    if (to_typed) {
        const int rc = validate_out_nodata(dtype, has_nodata, nodata);
        if (rc) return rc;
    }
    HK_ENTER(ctx);
    DevEnter entered(ctx, stream);
    Slot& sl = ctx->slots[stream];
    if (to_typed)
        HK_HIP(hk::launch_cast_out(dtype, {.in = src_dev, .in_stride = src_stride, .out = dst_dev, .out_stride = dst_stride,
                                           .height = height, .width = width, .has_nodata = has_nodata, .nodata = nodata}, sl.stream));
    else
        HK_HIP(hk::launch_cast_in(dtype, {.in = src_dev, .in_stride = src_stride, .out = dst_dev, .out_stride = dst_stride,
                                          .height = height, .width = width}, sl.stream));
    HK_HIP(hipStreamSynchronize(sl.stream));
    return HK_OK;
}

int hk_event_create(hk_ctx* ctx, hk_event** ev) {
    if (!ctx || !ev) return fail(HK_ERR_ARG, "NULL argument");
    HK_ENTER(ctx);
    hk_event* e = new (std::nothrow) hk_event();
    if (!e) return fail(HK_ERR_NOMEM, "out of host memory");
    hipError_t he = hipEventCreate(&e->ev);
    if (he != hipSuccess) {
        delete e;
        return fail(HK_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(he));
    }
    *ev = e;
    return HK_OK;
}
int hk_event_destroy(hk_ctx* ctx, hk_event* ev) {
    if (!ctx || !ev) return HK_OK;
    (void)hipEventDestroy(ev->ev);
    delete ev;
    return HK_OK;
}
int hk_event_record(hk_ctx* ctx, hk_event* ev, int32_t stream) {
    if (!ctx || !ev) return fail(HK_ERR_ARG, "NULL argument");
    if (const int bad = check_stream(ctx, stream)) return bad;
    HK_HIP(hipEventRecord(ev->ev, ctx->slots[stream].stream));
    return HK_OK;
}
int hk_stream_wait_event(hk_ctx* ctx, int32_t stream, hk_event* ev) {
    if (!ctx || !ev) return fail(HK_ERR_ARG, "NULL argument");
    if (const int bad = check_stream(ctx, stream)) return bad;
    HK_ENTER(ctx);
    HK_HIP(hipStreamWaitEvent(ctx->slots[stream].stream, ev->ev, 0));
    return HK_OK;
}
int hk_event_elapsed_ms(hk_ctx* ctx, hk_event* start, hk_event* stop, float* ms) {
    if (!ctx || !start || !stop || !ms) return fail(HK_ERR_ARG, "NULL argument");
    HK_HIP(hipEventSynchronize(stop->ev));
    HK_HIP(hipEventElapsedTime(ms, start->ev, stop->ev));
    return HK_OK;
}
int hk_stream_sync(hk_ctx* ctx, int32_t stream) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    if (const int bad = check_stream(ctx, stream)) return bad;
    HK_HIP(hipStreamSynchronize(ctx->slots[stream].stream));
    return HK_OK;
}

int hk_selftest(hk_ctx* ctx) {
    if (!ctx) return fail(HK_ERR_ARG, "ctx is NULL");
    HK_ENTER(ctx);
    int* d = nullptr;
    HK_HIP(dev_malloc(reinterpret_cast<void**>(&d), sizeof(int)));
    int code = -1;
    // on the transfer slot, one caller at a time: the pooled streams and their pinned words belong to leased / device-job calls
    // (PIN_WORD of slot 0 is where hk_inpaint_dev_counts reads a band's failure count from)
    std::lock_guard<std::mutex> lk(ctx->xfer_mu);
    Slot& xs = ctx->xfer;
    hipError_t e = hipMemsetAsync(d, 0, sizeof(int), xs.stream);
    if (e == hipSuccess) e = hk::launch_selftest(d, xs.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(xs.pin<int>(Slot::PIN_WORD), d, sizeof(int), hipMemcpyDeviceToHost, xs.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(xs.stream);
    if (e == hipSuccess) code = *xs.pin<int>(Slot::PIN_WORD);
    (void)dev_free(d);  // on every path
    if (e != hipSuccess) return fail(HK_ERR_HIP, "self-test launch failed: %s", hipGetErrorString(e));
    if (code != 0) return fail(HK_ERR_HIP, "cross-lane self-test failed (code 0x%x)", code);
    return HK_OK;
}

}  // extern "C"
