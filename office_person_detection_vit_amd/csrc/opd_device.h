// opd_device.h — PRIVATE header of libopd_hip: what every handle (detector, Re-ID, optical flow, floor map, the handle-less colour call)
// needs from the device short of its own kernels: the error macros, the entry-point lock and the graph guard, device selection, the pointer
// check, the page-locked / device staging pair, stream capture and the graph slot that a handle's cache is made of, the per-launch timer of
// the profiling modes, a holder of temporary device memory, and api_call: the wrapper (lock, then catch-all) that every function of
// include/opd_detr.h is defined through (its lock-free form, api_call_unlocked, is opd_host.h's: opd_host.cpp builds without HIP).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <exception>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/opd_detr.h"
#include "opd_host.h"

#define HIPCHK(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t _e = (expr);                                                                                \
        if (_e != hipSuccess)                                                                                  \
            return opd::fail(OPD_EHIP, std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + \
                                           ":" + std::to_string(__LINE__) + ")");                              \
    } while (0)

#define RCCHK(expr)            \
    do {                       \
        int _rc = (expr);      \
        if (_rc != 0) return _rc; \
    } while (0)

extern thread_local const char* opd_last_kernel_name;   // (opd_kernels.h: OPD_LAUNCH notes the kernel it launches)

namespace opd {

// Stream capture and other threads: the Python shim drives several handles from worker threads (HipDetrDetector(streams=N)).
// ROCm invalidates a capture in progress when ANOTHER thread allocates or frees memory, pins host memory or runs its
// one-time eager setup meanwhile, even in thread-local capture mode ("operation failed due to a previous error during
// capture").  Every entry point therefore holds this lock shared; a capture takes it exclusively for its few milliseconds.
// (g_api_mu and tl_api_lock: declared in opd_host.h, defined in opd_host.cpp)
// Handle churn and captured graphs.  Round 2 saw replays of a graph captured BEFORE another handle was destroyed and a third one
// created give wrong (finite or NaN) outputs, while the same launches issued eagerly stayed bit-exact; re-capturing after every
// handle creation / destruction (this epoch) made the symptom go away.  Round 3 went after the cause (profiles/r03_graph_churn_*.txt,
// tools/graph_churn_probe.py, tools/fresh_box_probe.sh) and did NOT find one:
//   * the round-2 binary with the guard patched out reproduced the corruption ONCE (first GPU process of a freshly acquired box) and
//     then 0 times in 22 further runs, 17 of them as the first GPU process of a fresh container; HEAD with the guard off: 0 of 26;
//   * per-launch checksum taps captured INTO the graph (opd_test_set_taps) never differed between capture run and replay;
//   * with every device buffer pre-filled with 0x00 / 0xFF and fenced by 256-KiB red zones (opd_test_set_alloc_poison) outputs are
//     bit-identical to an unpoisoned handle and every red zone stays intact, at HEAD and at the round-2 revision: no kernel reads
//     memory it has not written or writes next to its buffers (tests/test_workloads_gpu.py keeps this under test);
//   * foreign allocations between capture and replay (torch's caching allocator: 1 GiB of NaNs allocated, freed to the driver,
//     re-allocated; an RCCL communicator created and destroyed), pinned or pageable staging, captured memset nodes: no effect.
// Round 4 read the one bad log instead of provoking more (profiles/r03_graph_churn_bisect.txt: both replays of handle A after the churn
// differ from before by the SAME 4.198907): the CPU oracle gives max |logits_A(probe frames) - logits_B(golden frames)| = 4.2078 for
// handle B = the sharp-weights handle created during the churn, run on ITS frames -- equal to the recorded value within the fp16 noise
// of the device logits (|dlogit| ~ 1e-2), and no other candidate comes close (A's weights on the capture-time frames: 2.48, B's weights on
// A's frames: 3.34).  So the replay did not read stale weights, plans or pixels through A's baked pointers: A's caller got B's RESULTS,
// i.e. A's output buffers held what B's eager forward had written and A's replay wrote nothing over them -- device memory handed to B
// while A still owned it, or a dropped replay, below this library (every address baked into A's graph belongs to A or to A's weight
// set; neither is freed while A lives; red zones and poison runs rule out this library's kernels writing outside their buffers).  Nothing
// the capture code does wrong was found: launch errors inside a capture surface as the call's error (enqueue_forward's return code), and
// since round 4 a refused capture / instantiation does too instead of falling back to eager launches silently.
// Round 5 connected the log to round 4's own finding (counted waits that let register loads fly in front of LDS-DMA data prove nothing on this
// hardware): tools/scan_dma_waits.py over the ISA of the revision that produced the bad log (f889722; profiles/r05_scan_dma_waits_round2_revision.txt)
// finds 14 of its 20 barriers with LDS-DMA data in flight UNSOUND -- the first barrier of every fused-tail instantiation (six requests, then four
// or eight bias loads, `vmcnt(4)` / `vmcnt(8)`), gemm_ln256_kernel, gemm_ln256_os_kernel, three of the FFN kernel -- all on the path of that
// forward, and the one reproduction was the first GPU process of a freshly acquired box, i.e. cold requests, exactly when a request loses the
// race against a younger load.  So that binary COULD compute on LDS bytes that had not landed; HEAD cannot (0 of 157 such barriers, both element
// types, no kernel exempted; tests/test_isa_cpu.py).  What the scan does not explain is the VALUE: the same wrong number on two replays, equal to
// handle B's result within fp16 noise -- stale LDS bytes would have to be B's tiles, left in the CUs' LDS by B's forward just before, which is
// possible (LDS is not cleared between workgroups) but not shown.  Verdict: a sufficient mechanism existed at that revision and is gone; the
// "below the HIP API" reading is no longer needed to explain the log, nor excluded by it.  The guard stays ON (it costs one re-capture per
// handle creation / destruction, nothing per forward) and is no longer called load-bearing: the regression test
// test_graph_replay_survives_foreign_allocations_and_handle_churn runs with the guard OFF at HEAD and passes (round-5 GPU suite).
extern std::atomic<unsigned> g_handle_epoch;
extern std::atomic<int> g_graph_guard;   // opd_test_set_graph_guard(0): leave stale-epoch graphs alone (diagnosis only)
struct ApiScope {   // held by api_call around the body of every HIP-calling entry point; entry points calling each other nest harmlessly
    std::shared_lock<std::shared_mutex> lk;
    bool outer;
    ApiScope() : lk(g_api_mu, std::defer_lock), outer(tl_api_lock == nullptr) {
        if (outer) { lk.lock(); tl_api_lock = &lk; }
    }
    ~ApiScope() { if (outer) tl_api_lock = nullptr; }
};
struct ApiUnlocked {   // a blocking host wait inside an entry point (an event of another rank's making): the shared hold is dropped meanwhile
    std::shared_lock<std::shared_mutex>* s;
    ApiUnlocked() : s(tl_api_lock && tl_api_lock->owns_lock() ? tl_api_lock : nullptr) { if (s) s->unlock(); }
    ~ApiUnlocked() { if (s) s->lock(); }
};
struct CaptureExclusive {   // the calling thread's shared hold is handed back for the duration
    std::shared_lock<std::shared_mutex>* s;
    CaptureExclusive() : s(tl_api_lock) { if (s) s->unlock(); g_api_mu.lock(); }
    ~CaptureExclusive() { g_api_mu.unlock(); if (s) s->lock(); }
};

inline bool graph_stale(unsigned epoch) { return g_graph_guard.load() && epoch != g_handle_epoch.load(); }   // captured before handles came or went

// Capture the launches `body` enqueues on `stream` (thread-local mode, alone among the entry points) and instantiate them as *out.  A failing
// body is the call's error.  A refused capture or instantiation is an ERROR of the call too, not a reason to go on eagerly without saying so
// (round 3 did): the caller asked for the graph path, and a runtime that rejects the recorded launch sequence has a reason a caller should see.
template <typename F>
int capture_graph(hipStream_t stream, const char* what, F&& body, hipGraphExec_t* out) {
    *out = nullptr;
    hipGraph_t graph = nullptr;
    int rc;
    hipError_t ec;
    {
        CaptureExclusive alone;
        HIPCHK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        rc = body();
        ec = hipStreamEndCapture(stream, &graph);
    }
    if (rc != OPD_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ec == hipSuccess && graph) {
        ec = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ec == hipSuccess) return OPD_OK;
        (void)hipGetLastError();
        return fail(OPD_EHIP, std::string("hipGraphInstantiate refused ") + what + ": " + hipGetErrorString(ec) + " (OPD_FLAG_NO_GRAPH runs eagerly)");
    }
    (void)hipGetLastError();
    return fail(OPD_EHIP, std::string("hipStreamEndCapture refused ") + what + ": " + hipGetErrorString(ec) + " (OPD_FLAG_NO_GRAPH runs eagerly)");
}

// One cached graph: the executable and the handle epoch it was captured under.  run() drops a stale executable, captures `body` when the slot
// is empty, stamps the epoch and launches.  Which slot a call uses, and when it may capture at all, is the owner's policy.
struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    unsigned epoch = 0;
    void drop() {
        if (exec) (void)hipGraphExecDestroy(exec);
        exec = nullptr;
    }
    bool ready() {   // handles came or went since the capture: capture again (see g_handle_epoch)
        if (exec && graph_stale(epoch)) drop();
        return exec != nullptr;
    }
    template <typename F>
    int run(hipStream_t stream, const char* what, F&& body) {
        if (!ready()) {
            RCCHK(capture_graph(stream, what, body, &exec));
            epoch = g_handle_epoch.load();
        }
        HIPCHK(hipGraphLaunch(exec, stream));
        return OPD_OK;
    }
};

// How every function of include/opd_detr.h that calls HIP is defined: its braces hold one statement,
//     int opd_x(args) { return api_call("opd_x", [&]() -> int {
//         ... the body, at a function's usual indentation ...
//     }); }
// The shared hold of the entry-point lock first, then the body under the catch-all (opd_host.h: api_call_unlocked, which the entries
// without a HIP call use directly).  A `void` entry discards the code: its exception is swallowed.  tests/test_host_cpu.py holds every
// function of the header to this form.
template <typename F>
int api_call(const char* name, F&& body, bool create = false) {
    ApiScope api_scope;
    return api_call_unlocked(name, body, create);
}

// Per-launch timing of eager launches (the detector's profiling mode 1, the Re-ID handle's kernel-table hook): begin() and end() bracket
// a launch with two events of a pool that only grows, and note its class, the kernel the launcher named (OPD_LAUNCH) and its FLOPs.
struct KernelRow { std::string name; int launches; float ms; double flops; };
struct LaunchTimer {
    struct Mark { int cls; const char* name; double flops; hipEvent_t e0, e1; float ms; };   // ms: filled by fold(), < 0 where unreadable
    std::vector<hipEvent_t> pool;
    size_t cursor = 0;
    std::vector<Mark> marks;
    int begin(hipStream_t s, int cls, double flops) {
        while (pool.size() < cursor + 2) {
            hipEvent_t e;
            HIPCHK(hipEventCreate(&e));
            pool.push_back(e);
        }
        HIPCHK(hipEventRecord(pool[cursor], s));
        marks.push_back({cls, nullptr, flops, pool[cursor], pool[cursor + 1], -1.f});
        cursor += 2;
        opd_last_kernel_name = nullptr;
        return OPD_OK;
    }
    int end(hipStream_t s) {
        HIPCHK(hipEventRecord(marks.back().e1, s));
        marks.back().name = opd_last_kernel_name;   // what the launcher just launched: the name rocprofv3 prints, minus namespace and signature
        return OPD_OK;
    }
    void reset() { marks.clear(); cursor = 0; }   // the events are reused
    void release() {                              // (the owner has drained its stream)
        reset();
        for (hipEvent_t e : pool) (void)hipEventDestroy(e);
        pool.clear();
    }
    // The marks (their launches have completed) summed per kernel name into `rows`, appending to the rows already there in first-seen
    // order; a launch whose launcher named no kernel counts under unnamed[cls].  Returns how many marks could not be read (left out).
    int fold(std::vector<KernelRow>* rows, const char* const* unnamed) {
        int unread = 0;
        for (Mark& mk : marks) {
            if (hipEventElapsedTime(&mk.ms, mk.e0, mk.e1) != hipSuccess) { (void)hipGetLastError(); mk.ms = -1.f; ++unread; continue; }
            const char* nm = mk.name ? mk.name : unnamed[mk.cls];
            KernelRow* row = nullptr;
            for (auto& r : *rows)
                if (r.name == nm) { row = &r; break; }
            if (!row) { rows->push_back({nm, 0, 0.f, 0.0}); row = &rows->back(); }
            row->launches += 1; row->ms += mk.ms; row->flops += mk.flops;
        }
        return unread;
    }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A pointer that kernels will dereference must be memory the HIP runtime knows as device-accessible (device, page-locked host or managed):
// an ordinary host pointer handed over with a DEVICE mem_kind would make a kernel fault the GPU -- for every process on it -- instead of
// returning an error (hipPointerGetAttributes: 0.06 us per call).
inline bool device_accessible(const void* p) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged;
}

// Make `ordinal` the calling thread's device, or say why not on behalf of entry point `who` (`range_text`: the caller's own wording for an
// ordinal out of range)
inline int use_device(const char* who, int ordinal, const char* range_text = nullptr) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(OPD_EHIP, "no HIP device visible (this library has no CPU fallback)");
    if (ordinal < 0 || ordinal >= ndev) return fail(OPD_EINVAL, range_text ? std::string(range_text) : std::string(who) + ": no device " + std::to_string(ordinal));
    HIPCHK(hipSetDevice(ordinal));
    return OPD_OK;
}

// One step of making a handle (a stream, an allocation, the upload of its tables): OPD_ENOMEM "<who>: <what> failed: <the runtime's text>"
inline int made(const char* who, const char* what, hipError_t e) {
    if (e == hipSuccess) return OPD_OK;
    (void)hipGetLastError();
    return fail(OPD_ENOMEM, std::string(who) + ": " + what + " failed: " + hipGetErrorString(e));
}

// A page-locked host image and a device buffer that a handle stages its calls through.  reserve() makes each side at least as large as asked
// (0: that side is not needed); the growth policy is the caller's, in the byte counts it asks for.  A side that must grow is freed and
// allocated anew once the work on `s` has drained; *moved (nullable) then tells the caller to drop whatever holds the old addresses
// (captured graphs) before it launches anything.
struct Staging {
    uint8_t* host = nullptr;
    uint8_t* dev = nullptr;
    size_t host_cap = 0, dev_cap = 0;
    int reserve(const char* who, size_t host_bytes, size_t dev_bytes, hipStream_t s, bool* moved = nullptr) {
        const bool grow_host = host_bytes > host_cap, grow_dev = dev_bytes > dev_cap;
        if (moved) *moved = grow_host || grow_dev;   // set before anything is freed: true also when the regrow then fails
        if (!grow_host && !grow_dev) return OPD_OK;
        HIPCHK(hipStreamSynchronize(s));
        if (grow_host) {
            if (host) (void)hipHostFree(host);
            host = nullptr; host_cap = 0;
            void* p = nullptr;
            RCCHK(made(who, "page-locked allocation", hipHostMalloc(&p, host_bytes, hipHostMallocDefault)));
            host = static_cast<uint8_t*>(p);
            host_cap = host_bytes;
        }
        if (grow_dev) {
            if (dev) (void)hipFree(dev);
            dev = nullptr; dev_cap = 0;
            void* p = nullptr;
            RCCHK(made(who, "staging allocation", hipMalloc(&p, dev_bytes)));
            dev = static_cast<uint8_t*>(p);
            dev_cap = dev_bytes;
        }
        return OPD_OK;
    }
    void release() {   // (the owner has drained its stream)
        if (host) (void)hipHostFree(host);
        if (dev) (void)hipFree(dev);
        host = dev = nullptr; host_cap = dev_cap = 0;
    }
};

// Device memory that lives as long as this object: temporaries of a call (opd_similarity_matrix) and the buffers of the kernel-level test hooks
struct DevMem {
    std::vector<void*> ptrs;
    bool ok = true;   // false once an allocation or copy has failed (alloc() / up() returned nullptr)
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { for (void* p : ptrs) (void)hipFree(p); }
    // `count` elements, uninitialised, with 16 bytes of slack behind them
    template <typename T>
    T* alloc(size_t count) {
        void* d = nullptr;
        if (hipMalloc(&d, count * sizeof(T) + 16) != hipSuccess) { ok = false; return nullptr; }
        ptrs.push_back(d);
        return static_cast<T*>(d);
    }
    // ... holding a copy of host[0, count) (a null host: left uninitialised)
    template <typename T>
    T* up(const T* host, size_t count) {
        T* d = alloc<T>(count);
        if (d && host && hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { ok = false; return nullptr; }
        return d;
    }
    // the same by bytes, zeroed for a null host
    void* up_bytes(const void* host, size_t bytes) {
        uint8_t* d = up(static_cast<const uint8_t*>(host), bytes);
        if (d && !host && bytes && hipMemset(d, 0, bytes) != hipSuccess) { ok = false; return nullptr; }
        return d;
    }
};

}  // namespace opd
