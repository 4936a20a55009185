// aeron_cluster_amd.cpp — host side of the reference codec surface over the C ABI.
// Host memory in, host memory out (the reference's API contract).  Every batch call runs a
// chunk pipeline: the batch is cut into chunks of a few MiB; the host threads stage chunk k+1 in
// page-locked memory while chunk k is copied to HBM (copy-in stream), coded by the HIP kernels of
// include/sbecodec.h (compute stream) and chunk k-1 is copied back (copy-out stream).  Encoded
// bytes land by DMA directly in a recycled page-locked block the caller receives (HostBytes);
// decode descriptors land in one the same way, and ParseResults are built from them on the host
// threads.  Results are materialised from the device descriptors (views into the caller's own
// bytes), never recomputed here.
#include "aeron_cluster_amd.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <ctime>
#include <iomanip>
#include <iostream>
#include <map>
#include <mutex>
#include <random>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include "sbecodec.h"
#include "workers.hpp"

namespace aeron_cluster {

// ======================================================================================
// host runtime: worker threads, page-locked block pool
// ======================================================================================
namespace {

[[noreturn]] void fail(const char* what) {
    throw std::runtime_error(std::string("sbecodec: ") + what + " (" + sbe_last_error() + ")");
}

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("sbecodec: ") + what + ": " + hipGetErrorString(e));
}

using detail::Workers;  // the worker pool (workers.hpp)

// parallel_for over [0, n) in contiguous ranges of at least `grain` items: fn(lo, hi).
template <class F>
void for_ranges(size_t n, size_t grain, F&& fn) {
    Workers& w = Workers::get();
    const size_t maxt = (size_t)w.size() * 4;
    size_t ntasks = std::min(maxt, std::max<size_t>(1, n / std::max<size_t>(grain, 1)));
    if (ntasks <= 1) {
        if (n) fn(size_t(0), n);
        return;
    }
    w.parallel_for(ntasks, [&](size_t t) { fn(n * t / ntasks, n * (t + 1) / ntasks); });
}

// The page-locked ranges this library knows: its own pool blocks and staging buffers and the
// ranges the caller registered with host_register, each with its device address (looked up once,
// when the range is added).  A per-call lookup here replaces the HIP pointer queries, which cost
// microseconds per call.
class PinnedRegistry {
public:
    static PinnedRegistry& get() {
        static PinnedRegistry* r = new PinnedRegistry();  // never destroyed
        return *r;
    }
    void add(const void* p, size_t bytes) {
        void* d = nullptr;
        if (hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) {
            (void)hipGetLastError();
            d = nullptr;
        }
        std::lock_guard<std::mutex> g(m_);
        ranges_[reinterpret_cast<uintptr_t>(p)] = Range{reinterpret_cast<uintptr_t>(p) + bytes, reinterpret_cast<uintptr_t>(d)};
    }
    void remove(const void* p) {
        std::lock_guard<std::mutex> g(m_);
        ranges_.erase(reinterpret_cast<uintptr_t>(p));
    }
    // [p, p + bytes) inside one known range: its device address (nullptr when it has none), true
    bool find(const void* p, size_t bytes, uint8_t** dev) const {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        std::lock_guard<std::mutex> g(m_);
        auto it = ranges_.upper_bound(a);
        if (it == ranges_.begin()) return false;
        --it;
        if (a + bytes > it->second.end) return false;
        *dev = it->second.dev ? reinterpret_cast<uint8_t*>(it->second.dev + (a - it->first)) : nullptr;
        return true;
    }

private:
    struct Range {
        uintptr_t end, dev;
    };
    mutable std::mutex m_;
    std::map<uintptr_t, Range> ranges_;
};

// Page-locked host blocks recycled by size class (powers of two from 4 KiB); hipHostMalloc costs
// milliseconds per call for large blocks, so a block is allocated once and reused.  Free blocks are
// kept up to AERON_AMD_PINNED_CACHE_BYTES (default 4 GiB) in all; a block returned beyond that is
// freed.  Blocks held by callers (EncodedBatch, ParsedBatch) do not count against the cap.
class PinnedPool {
public:
    static PinnedPool& get() {
        static PinnedPool* p = new PinnedPool();  // never destroyed (blocks may outlive statics)
        return *p;
    }
    std::shared_ptr<void> take(size_t bytes) {
        size_t cls = size_t(1) << 12;
        while (cls < bytes) cls <<= 1;
        void* p = nullptr;
        {
            std::lock_guard<std::mutex> g(m_);
            auto& fl = free_[cls];
            if (!fl.empty()) {
                p = fl.back();
                fl.pop_back();
                cached_ -= cls;
            }
        }
        if (!p) {
            hip_check(hipHostMalloc(&p, cls, hipHostMallocDefault), "hipHostMalloc");
            PinnedRegistry::get().add(p, cls);
        }
        return std::shared_ptr<void>(p, [this, cls](void* q) { give(q, cls); });
    }

private:
    void give(void* p, size_t cls) {
        {
            std::lock_guard<std::mutex> g(m_);
            if (cached_ + cls <= max_cached_) {
                free_[cls].push_back(p);
                cached_ += cls;
                return;
            }
        }
        PinnedRegistry::get().remove(p);
        (void)hipHostFree(p);
    }
    PinnedPool() {
        if (const char* e = std::getenv("AERON_AMD_PINNED_CACHE_BYTES")) max_cached_ = (size_t)std::max(0LL, std::atoll(e));
    }
    size_t max_cached_ = size_t(4) << 30;
    std::mutex m_;
    std::map<size_t, std::vector<void*>> free_;
    size_t cached_ = 0;
};

// Growable device / page-locked buffer owned by one thread's context.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    void need(size_t n) {
        if (n <= cap) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t c = n < 4096 ? 4096 : n + n / 4;
        hip_check(hipMalloc(&p, c), "hipMalloc");
        cap = c;
    }
    uint8_t* b() const { return static_cast<uint8_t*>(p); }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
struct HostBuf {
    void* p = nullptr;
    uint8_t* dev = nullptr;  // its device address (the zero-copy kernels read it there)
    size_t cap = 0;
    void need(size_t n) {
        if (n <= cap) return;
        release();
        const size_t c = n < 4096 ? 4096 : n + n / 4;
        hip_check(hipHostMalloc(&p, c, hipHostMallocDefault), "hipHostMalloc");
        cap = c;
        PinnedRegistry::get().add(p, c);
        uint8_t* d = nullptr;
        PinnedRegistry::get().find(p, 1, &d);
        dev = d;
    }
    uint8_t* b() const { return static_cast<uint8_t*>(p); }
    void release() {
        if (p) {
            PinnedRegistry::get().remove(p);
            (void)hipHostFree(p);
        }
        p = nullptr;
        dev = nullptr;
        cap = 0;
    }
    ~HostBuf() { release(); }
};

// Three-stream chunk pipeline: host→device copies, kernels and device→host copies each on a
// stream of their own, ordered per chunk by events, so that chunk k+1's H2D, chunk k's kernels and
// chunk k-1's D2H run at once (on one stream the copy engine serialises H2D behind D2H).  Chunk k
// uses slot k % kSlots: its page-locked staging buffer and its device buffers.
struct Pipeline {
    static constexpr int kSlots = 3;
    struct Slot {
        hipEvent_t in_done = nullptr, comp_done = nullptr, out_done = nullptr;
        bool used = false;  // its events were recorded by an earlier chunk
        HostBuf pin;
        DevBuf d_in, d_out;
    };
    hipStream_t s_in = nullptr, s_comp = nullptr, s_out = nullptr;
    Slot slot[kSlots];
    // one-chunk calls: copy-in, kernels and copy-out in order on the compute stream, no events
    // (a small batch is latency-bound: each event record / wait costs more than it overlaps)
    bool serial = false;
    // called before the first copy or kernel of a batch is enqueued (Ctx: stop the resident server)
    void (*before_enqueue)(void*) = nullptr;
    void* before_arg = nullptr;
    void enqueue_hook() {
        if (before_enqueue) before_enqueue(before_arg);
    }

    void create() {
        for (hipStream_t* st : {&s_in, &s_comp, &s_out})
            hip_check(hipStreamCreateWithFlags(st, hipStreamNonBlocking), "hipStreamCreate");
        for (Slot& sl : slot)
            for (hipEvent_t* e : {&sl.in_done, &sl.comp_done, &sl.out_done})
                hip_check(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate");
    }
    void destroy() {
        for (Slot& sl : slot)
            for (hipEvent_t e : {sl.in_done, sl.comp_done, sl.out_done})
                if (e) (void)hipEventDestroy(e);
        for (hipStream_t st : {s_in, s_comp, s_out})
            if (st) (void)hipStreamDestroy(st);
    }
    // chunk k's slot, once the host may rewrite its staging buffer (its last H2D is done)
    Slot& begin(size_t k) {
        Slot& sl = slot[serial ? 0 : k % kSlots];
        if (sl.used) hip_check(hipEventSynchronize(sl.in_done), "hipEventSynchronize");
        return sl;
    }
    void drain() {
        if (serial) {
            hip_check(hipStreamSynchronize(s_comp), "hipStreamSynchronize");
            return;
        }
        for (hipStream_t st : {s_in, s_comp, s_out}) hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
    // device buffers of the slot at least this large (growing drains the pipeline first: the old
    // buffers may still be in use by queued work)
    void reserve(Slot& sl, size_t in_bytes, size_t out_bytes) {
        if (in_bytes <= sl.d_in.cap && out_bytes <= sl.d_out.cap) return;
        drain();
        sl.d_in.need(in_bytes);
        sl.d_out.need(out_bytes);
    }
    // the slot's staged bytes to d_in, plus (direct) `dbytes` page-locked caller bytes to d_in + doff
    void copy_in(Slot& sl, size_t bytes, const void* direct = nullptr, size_t doff = 0, size_t dbytes = 0) {
        enqueue_hook();
        hipStream_t st = serial ? s_comp : s_in;
        if (!serial && sl.used) hip_check(hipStreamWaitEvent(s_in, sl.comp_done, 0), "hipStreamWaitEvent");  // d_in read
        hip_check(hipMemcpyAsync(sl.d_in.p, sl.pin.p, bytes, hipMemcpyHostToDevice, st), "H2D");
        if (dbytes) hip_check(hipMemcpyAsync(sl.d_in.b() + doff, direct, dbytes, hipMemcpyHostToDevice, st), "H2D");
        if (!serial) hip_check(hipEventRecord(sl.in_done, s_in), "hipEventRecord");
    }
    // the stream to launch the chunk's kernels on (after its input copy and the slot's last D2H)
    hipStream_t compute(Slot& sl) {
        enqueue_hook();
        if (serial) return s_comp;
        hip_check(hipStreamWaitEvent(s_comp, sl.in_done, 0), "hipStreamWaitEvent");
        if (sl.used) hip_check(hipStreamWaitEvent(s_comp, sl.out_done, 0), "hipStreamWaitEvent");
        return s_comp;
    }
    // the stream to issue the chunk's D2H copies on (after its kernels)
    hipStream_t copy_out(Slot& sl) {
        if (serial) return s_comp;
        hip_check(hipEventRecord(sl.comp_done, s_comp), "hipEventRecord");
        hip_check(hipStreamWaitEvent(s_out, sl.comp_done, 0), "hipStreamWaitEvent");
        return s_out;
    }
    void end(Slot& sl) {
        if (serial) return;
        hip_check(hipEventRecord(sl.out_done, s_out), "hipEventRecord");
        sl.used = true;
    }
};

// Batches of at most this many records (and within the zero-copy size) go to the thread's serve
// kernel (sbe_server_*: a resident wave polling a page-locked request slot, no launch per call);
// larger ones to the batch kernels.  One wave walks a served batch tile by tile, so the batch
// kernels overtake it between 64 and 256 fixed-256 records (profiles/r04_host_latency_serve.log:
// 64 records served 16.8 / 10.1 µs encode / decode against 24.2 / 18.8 µs launched, 256 records
// 50.0 / 28.6 against 28.1 / 19.6).  AERON_AMD_SERVE_RECORDS overrides (0: never serve).
size_t serve_max_records() {
    static const size_t v = [] {
        const char* e = std::getenv("AERON_AMD_SERVE_RECORDS");
        const long long x = e ? std::atoll(e) : 96;
        return (size_t)std::min<long long>(std::max(0LL, x), SBE_SERVE_MAX_RECORDS);
    }();
    return v;
}

// Batches of up to this many records that the single wave does not take go to the server's other
// workgroups as a whole (decode: tile per workgroup; encode: the tile loop with tile sums from the
// host's plan) instead of a launch: AERON_AMD_SERVE_WIDE_RECORDS (0: never); the server has
// AERON_AMD_SERVE_WGS workgroups (default 32).
size_t serve_wide_max_records() {
    static const size_t v = [] {
        const char* e = std::getenv("AERON_AMD_SERVE_WIDE_RECORDS");
        const long long x = e ? std::atoll(e) : 4096;
        return (size_t)std::min<long long>(std::max(0LL, x), SBE_SERVE_MAX_RECORDS);
    }();
    return v;
}
uint32_t serve_workgroups() {
    static const uint32_t v = [] {
        const char* e = std::getenv("AERON_AMD_SERVE_WGS");
        const long long x = e ? std::atoll(e) : 32;
        return (uint32_t)std::min<long long>(std::max(1LL, x), SBE_SERVE_MAX_WORKGROUPS);
    }();
    return v;
}

// How long an idle serve kernel keeps polling before it exits (AERON_AMD_SERVE_IDLE_US, default
// 1 ms); the next small call relaunches it (one launch, ≈ 6-12 µs).  While it is resident, work
// that HIP maps to the same hardware queue waits behind it (streams share GPU_MAX_HW_QUEUES
// queues), as does any device-wide synchronisation: short is the safe default.
uint32_t serve_idle_us() {
    static const uint32_t v = [] {
        const char* e = std::getenv("AERON_AMD_SERVE_IDLE_US");
        return e ? (uint32_t)std::max(1LL, std::atoll(e)) : 1000u;
    }();
    return v;
}

// Per-thread device context (the reference's codec functions are reentrant statics).
struct Ctx {
    Pipeline pipe;
    DevBuf d_aux;   // reassembly / Order JSON
    DevBuf d_ws;    // encode workspace of the zero-copy path
    HostBuf h_aux;
    std::vector<uint64_t> pin, pout;  // encode plan scratch (kept: first-touch costs on every call otherwise)
    sbe_server* srv = nullptr;
    bool srv_failed = false;   // in a cool-down after a failure (server() returns nullptr)
    int srv_failures = 0;      // failures so far (the cool-down doubles with each)
    std::chrono::steady_clock::time_point srv_retry_at{};
    Ctx() {
        if (sbe_device_ready() != 1) fail("no gfx950 device visible");
        pipe.create();
        pipe.before_enqueue = [](void* self) { static_cast<Ctx*>(self)->quiesce(); };
        pipe.before_arg = this;
    }
    // the compute stream for a launch outside the chunk loop (the resident server stopped first)
    hipStream_t batch_stream() {
        quiesce();
        return pipe.s_comp;
    }
    ~Ctx() {
        if (srv) (void)sbe_server_destroy(srv);
        pipe.destroy();
    }
    // The serve kernel for a batch of n records, or nullptr (too large, disabled, or unavailable:
    // the batch kernels take it).
    // wide: a batch for several workgroups (up to serve_wide_max_records())
    sbe_server* server(size_t n, bool wide = false) {
        if (n == 0 || n > (wide ? serve_wide_max_records() : serve_max_records())) return nullptr;
        if (srv_failed) {
            if (std::chrono::steady_clock::now() < srv_retry_at) return nullptr;
            srv_failed = false;  // the cool-down is over: try a server again
        }
        if (!srv && sbe_server_create_wide(&srv, serve_idle_us(), serve_workgroups()) != SBE_OK) {
            srv = nullptr;
            (void)hipGetLastError();
            back_off();
        }
        return srv;
    }
    // A serve request failed (timed out, or the server's stream failed): the server is freed (a
    // bounded wait, sbe_server_destroy) and this thread's calls go to the batch kernels for a
    // cool-down that doubles with each failure of this thread, from 1 s up to 64 s; then a new server is
    // tried (one transient timeout no longer disables the serve path for good).
    void drop_server() noexcept {
        if (srv) (void)sbe_server_destroy(srv);
        srv = nullptr;
        (void)hipGetLastError();
        back_off();
    }
    void back_off() noexcept {
        srv_failed = true;
        srv_retry_at = std::chrono::steady_clock::now() + std::chrono::seconds(1ll << std::min(srv_failures, 6));
        ++srv_failures;
    }
    // Before batch work is enqueued on this thread's streams: a resident server of this thread
    // exits first (a shutdown request, then its stream drains), so that no kernel or copy of the
    // batch can wait behind it on a shared hardware queue.  Free when the server is not running;
    // the next small call relaunches it.
    void quiesce() noexcept {
        if (srv && sbe_server_quiesce(srv) != SBE_OK) drop_server();
    }
    void sync_all() { pipe.drain(); }
    // After a throw inside a chunk loop: wait for every copy and kernel already queued (their
    // page-locked sources and destinations must not go back to a pool, or be restaged, while a
    // DMA still reads or writes them), then forget the slots' event history.  Never throws.
    void abort_all() noexcept {
        for (hipStream_t st : {pipe.s_in, pipe.s_comp, pipe.s_out})
            if (st) (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        for (Pipeline::Slot& sl : pipe.slot) sl.used = false;
    }
};

// Drains the pipeline if a chunk loop unwinds (declared after the buffers the queued copies use, so
// it runs before they are released).
struct PipeGuard {
    Ctx& c;
    bool armed = true;
    explicit PipeGuard(Ctx& x) : c(x) {}
    ~PipeGuard() {
        if (armed) c.abort_all();
    }
    void release() { armed = false; }
};

// The device address of page-locked host memory (hipHostMalloc'd or registered), or nullptr when
// it has none: kernels of the zero-copy path read their input and write their results there.
// An interior pointer resolves through the start of its allocation; ranges this library knows
// (PinnedRegistry) need no HIP query.
void* device_view(const void* host) {
    uint8_t* d0 = nullptr;
    if (PinnedRegistry::get().find(host, 1, &d0)) return d0;
    void* start = nullptr;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR,
                               (hipDeviceptr_t)const_cast<void*>(host)) != hipSuccess || !start) {
        (void)hipGetLastError();
        return nullptr;
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, start, 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint8_t*>(d) + (static_cast<const uint8_t*>(host) - static_cast<const uint8_t*>(start));
}

// Batches up to this many staged bytes (one pipeline chunk) take the zero-copy path: the kernels
// read the page-locked staging buffer and write their results straight into the page-locked result
// block over PCIe, one launch (encode: two) and one completion wait, no hipMemcpyAsync.  Larger
// one-chunk batches, and every chunk of a multi-chunk batch, go through the DMA copy engines.
// AERON_AMD_ZC_BYTES overrides (0: never).
size_t zero_copy_max_bytes() {
    static const size_t v = [] {
        const char* e = std::getenv("AERON_AMD_ZC_BYTES");
        return e ? (size_t)std::max(0LL, std::atoll(e)) : (size_t(4) << 20);
    }();
    return v;
}

Ctx& ctx() {
    thread_local Ctx c;
    return c;
}

inline size_t al16(size_t x) { return (x + 15) & ~(size_t)15; }

// n bytes from src to dst for the short strings of a record (topic, type, uuid, headers: tens of
// bytes): fixed-size, overlapping moves that the compiler inlines, instead of a memcpy call per
// string (the call, not the bytes, was the cost of staging and of building ParseResults)
inline void copy_small(void* dst_, const void* src_, size_t n) {
    uint8_t* dst = static_cast<uint8_t*>(dst_);
    const uint8_t* src = static_cast<const uint8_t*>(src_);
    if (n > 64) {
        std::memcpy(dst, src, n);
    } else if (n >= 16) {
        for (size_t k = 0; k + 16 < n; k += 16) std::memcpy(dst + k, src + k, 16);
        std::memcpy(dst + n - 16, src + n - 16, 16);
    } else if (n >= 8) {
        std::memcpy(dst, src, 8);
        std::memcpy(dst + n - 8, src + n - 8, 8);
    } else if (n >= 4) {
        std::memcpy(dst, src, 4);
        std::memcpy(dst + n - 4, src + n - 4, 4);
    } else if (n) {
        dst[0] = src[0];
        dst[n / 2] = src[n / 2];
        dst[n - 1] = src[n - 1];
    }
}

// AERON_AMD_TRACE=1: one line per batch call on stderr with its phase times (diagnosis only)
struct Trace {
    using clk = std::chrono::steady_clock;
    bool on;
    const char* what;
    clk::time_point t0, last;
    double plan = 0, stage = 0, wait = 0, enqueue = 0, sync = 0, finish = 0;
    explicit Trace(const char* w) : on(enabled()), what(w) {
        if (on) t0 = last = clk::now();
    }
    static bool enabled() {
        static const bool e = [] {
            const char* v = std::getenv("AERON_AMD_TRACE");
            return v && v[0] == '1';
        }();
        return e;
    }
    void lap(double& acc) {
        if (!on) return;
        const clk::time_point t = clk::now();
        acc += std::chrono::duration<double, std::micro>(t - last).count();
        last = t;
    }
    void done(size_t n, size_t chunks) {
        if (!on) return;
        std::fprintf(stderr,
                     "[trace] t0=%.1f %s n=%zu chunks=%zu threads=%u total=%.1fus plan=%.1f stage=%.1f wait=%.1f enqueue=%.1f sync=%.1f "
                     "finish=%.1f\n",
                     std::chrono::duration<double, std::micro>(t0.time_since_epoch()).count(), what, n, chunks,
                     Workers::get().size(), std::chrono::duration<double, std::micro>(clk::now() - t0).count(), plan, stage,
                     wait, enqueue, sync, finish);
    }
};

// Bytes of staged work per pipeline chunk: AERON_AMD_CHUNK_BYTES when set, else a third of the
// batch's bytes within [8, 32] MiB (and at most 65536 records, chunk_records): every chunk pays its
// copies' and launches' fixed costs, and a batch of a few chunks still overlaps its copies.
// host_latency, fixed-256 records, encode + parse_batch, three interleaved repetitions per
// setting (profiles/r03_host_chunks.log): 8 MiB chunks 46 M rec/s at 262 K records (median) and
// 39 M at 1 M; 16 MiB chunks (65536 records) 48 / 43 M at 262 K and 53 / 58 M at 1 M.  This
// rule against fixed 8 MiB chunks, interleaved on one box: 262 K 43.5 vs 41.5 M, 1 M 48.3 vs
// 47.8 M (medians; the box-to-box and run-to-run spread of these host numbers is ~20 %).
size_t chunk_target_bytes(size_t total_bytes) {
    static const size_t env = [] {
        const char* e = std::getenv("AERON_AMD_CHUNK_BYTES");
        const long long x = e ? std::atoll(e) : 0;
        return x > 0 ? (size_t)x : size_t(0);
    }();
    if (env) return env;
    return std::min(size_t(32) << 20, std::max(size_t(8) << 20, total_bytes / 3));
}
// Records per chunk: a power of two so that a chunk holds about chunk_target_bytes().
size_t chunk_records(size_t n, size_t total_bytes) {
    const size_t avg = std::max<size_t>(1, total_bytes / std::max<size_t>(n, 1));
    const size_t target = chunk_target_bytes(total_bytes);
    size_t c = 1;
    while (c < n && c < 65536 && (c * 2) * avg <= target) c *= 2;
    return c;
}

// Exclusive prefix sums of per-item values produced by val(i), in parallel ranges: out[0..n].
template <class V>
void prefix(size_t n, std::vector<uint64_t>& out, V&& val) {
    out.resize(n + 1);
    Workers& w = Workers::get();
    const size_t ntasks = n < 65536 ? 1 : std::min<size_t>(w.size() * 2, n / 16384);
    std::vector<uint64_t> part(ntasks + 1, 0);
    auto lo = [&](size_t t) { return n * t / ntasks; };
    w.parallel_for(ntasks, [&](size_t t) {
        uint64_t s = 0;
        for (size_t i = lo(t); i < lo(t + 1); ++i) {
            out[i] = s;
            s += val(i);
        }
        part[t + 1] = s;
    });
    for (size_t t = 0; t < ntasks; ++t) part[t + 1] += part[t];
    w.parallel_for(ntasks, [&](size_t t) {
        if (part[t])
            for (size_t i = lo(t); i < lo(t + 1); ++i) out[i] += part[t];
    });
    out[n] = part[ntasks];
}

// Two exclusive prefix sums in one pass: val(i, x, y) gives item i's two values.
template <class V>
void prefix2(size_t n, std::vector<uint64_t>& ox, std::vector<uint64_t>& oy, V&& val) {
    ox.resize(n + 1);
    oy.resize(n + 1);
    Workers& w = Workers::get();
    const size_t ntasks = n < 32768 ? 1 : std::min<size_t>(w.size() * 2, n / 8192);
    std::vector<uint64_t> px(ntasks + 1, 0), py(ntasks + 1, 0);
    auto lo = [&](size_t t) { return n * t / ntasks; };
    w.parallel_for(ntasks, [&](size_t t) {
        uint64_t sx = 0, sy = 0;
        for (size_t i = lo(t); i < lo(t + 1); ++i) {
            uint64_t x, y;
            val(i, x, y);
            ox[i] = sx;
            oy[i] = sy;
            sx += x;
            sy += y;
        }
        px[t + 1] = sx;
        py[t + 1] = sy;
    });
    for (size_t t = 0; t < ntasks; ++t) {
        px[t + 1] += px[t];
        py[t + 1] += py[t];
    }
    w.parallel_for(ntasks, [&](size_t t) {
        if (t == 0) return;
        for (size_t i = lo(t); i < lo(t + 1); ++i) {
            ox[i] += px[t];
            oy[i] += py[t];
        }
    });
    ox[n] = px[ntasks];
    oy[n] = py[ntasks];
}

}  // namespace

namespace detail {
struct HostBytesAccess {
    template <class T = uint8_t>
    static HostArray<T> make(size_t n) {
        HostArray<T> h;
        if (n) {
            h.block_ = PinnedPool::get().take(n * sizeof(T));
            h.p_ = static_cast<T*>(h.block_.get());
        }
        h.n_ = n;
        return h;
    }
    // n elements at p inside `block` (several arrays of one result share a block)
    template <class T>
    static HostArray<T> view(const std::shared_ptr<void>& block, void* p, size_t n) {
        HostArray<T> h;
        h.block_ = block;
        h.p_ = n ? static_cast<T*>(p) : nullptr;
        h.n_ = n;
        return h;
    }
    template <class T>
    static void zero(HostArray<T>& h) {
        if (h.n_) std::memset(static_cast<void*>(h.p_), 0, h.n_ * sizeof(T));
    }
};

// Host copy of the decode descriptors, chunk-major: chunk c (records [c*C, c*C + C)) is the
// device's struct of arrays for C records, copied back as one block.
struct Descriptors {
    std::shared_ptr<void> block;
    size_t n = 0;
    unsigned shift = 0;  // C = 1 << shift
    size_t chunk_bytes = 0;
    size_t o_fl = 0, o_hdr = 0, o_ts = 0, o_off = 0, o_len = 0, o_seq = 0;
    bool has_seq = false;

    void layout(size_t C, bool seq) {
        shift = 0;
        while ((size_t(1) << shift) < C) ++shift;
        o_fl = al16(C);
        o_hdr = o_fl + al16(C);
        o_ts = o_hdr + al16(8 * C);
        o_off = o_ts + al16(8 * C);
        o_len = o_off + al16(20 * C);
        o_seq = o_len + al16(20 * C);
        chunk_bytes = o_seq + (seq ? al16(8 * C) : 0);
        has_seq = seq;
    }
    const uint8_t* base(size_t i) const {
        return static_cast<const uint8_t*>(block.get()) + (i >> shift) * chunk_bytes;
    }
    size_t j(size_t i) const { return i & ((size_t(1) << shift) - 1); }
    uint8_t status(size_t i) const { return base(i)[j(i)]; }
    uint8_t flags(size_t i) const { return base(i)[o_fl + j(i)]; }
    const uint16_t* hdr(size_t i) const { return reinterpret_cast<const uint16_t*>(base(i) + o_hdr) + 4 * j(i); }
    uint64_t ts(size_t i) const { return reinterpret_cast<const uint64_t*>(base(i) + o_ts)[j(i)]; }
    const uint32_t* off(size_t i) const { return reinterpret_cast<const uint32_t*>(base(i) + o_off) + 5 * j(i); }
    const uint32_t* len(size_t i) const { return reinterpret_cast<const uint32_t*>(base(i) + o_len) + 5 * j(i); }
    // ParseResult.sequence_number: the device evaluates it for flagged TopicMessages only
    // (include/sbecodec.h, sbe_decoded.seq); every other record's is 0
    uint64_t seq(size_t i) const {
        if (!has_seq || status(i) != SBE_ST_TM || !(flags(i) & (SBE_FL_SEQ_KEY | SBE_FL_SEQ_ESC))) return 0;
        return reinterpret_cast<const uint64_t*>(base(i) + o_seq)[j(i)];
    }
};
}  // namespace detail

using detail::Descriptors;
using detail::HostBytesAccess;

namespace {

// [p, p + bytes) inside one page-locked host allocation (hipHostMalloc, or memory registered with
// host_register, e.g. an Aeron term buffer, or a HostBytes of this library): the copy engines read
// it in place, with no staging copy.
bool page_locked(const void* p, size_t bytes) {
    if (!p || bytes == 0) return false;
    uint8_t* dev = nullptr;
    if (PinnedRegistry::get().find(p, bytes, &dev)) return true;
    // memory page-locked outside this library (the caller's own hipHostMalloc) is found by the HIP
    // pointer query, which costs microseconds: asked only where that is small against the copy
    if (bytes < (size_t(1) << 20)) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    void* start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)const_cast<void*>(p)) !=
            hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)const_cast<void*>(p)) !=
            hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return start && static_cast<const uint8_t*>(p) >= static_cast<const uint8_t*>(start) &&
           static_cast<const uint8_t*>(p) + bytes <= static_cast<const uint8_t*>(start) + size;
}

// Decode n records data[rec_off[i], rec_off[i+1]) with `mode` through the chunk pipeline.
// on_chunk(d, a, m), when given, runs on the calling thread for each chunk (records [a, a+m)) as
// soon as its descriptors are on the host, while the later chunks are still being copied and
// decoded: the host's work on chunk k overlaps the device's on chunk k+1.
using ChunkFn = std::function<void(const Descriptors&, size_t, size_t)>;

// The zero-copy path of a one-chunk decode: the offsets (and, unless the caller's bytes are
// page-locked already, the records) staged in the slot's page-locked buffer, which the kernel reads
// over PCIe; the descriptors written by the kernel straight into d.block.  One launch, one wait.
// false (nothing launched) when some buffer has no device address.
bool decode_zero_copy(Ctx& c, const uint8_t* data, const uint64_t* rec_off, size_t n, uint32_t mode, bool direct,
                      Descriptors& d) {
    Pipeline& P = c.pipe;
    Pipeline::Slot& sl = P.slot[0];  // serial use (the pipeline is idle between calls)
    const uint64_t lo = rec_off[0], bytes = rec_off[n] - lo;
    const size_t o_data = al16((n + 1) * 8);
    const bool parse = mode == SBE_DEC_PARSE_MESSAGE;
    // small batches: the serve kernel, inputs straight from the caller's memory into its request slot
    if (sbe_server* srv = c.server(n); srv && o_data + bytes <= SBE_SERVE_INLINE_BYTES) {
        uint8_t* dblk = static_cast<uint8_t*>(device_view(d.block.get()));
        if (dblk) {
            sbe_decoded out{dblk,
                            dblk + d.o_fl,
                            reinterpret_cast<uint16_t*>(dblk + d.o_hdr),
                            reinterpret_cast<uint64_t*>(dblk + d.o_ts),
                            reinterpret_cast<uint32_t*>(dblk + d.o_off),
                            reinterpret_cast<uint32_t*>(dblk + d.o_len),
                            parse ? reinterpret_cast<uint64_t*>(dblk + d.o_seq) : nullptr};
            if (sbe_serve_decode_host(srv, data, rec_off, n, mode, &out) == SBE_OK) return true;
            c.drop_server();  // the batch kernels take this call and every later one
        }
    }
    // the kernel reads its records from a 16-B aligned base: page-locked caller bytes are read from
    // the 16-B boundary below the first record (offsets rebased to it); staged bytes start aligned
    const uint64_t base = direct ? (lo & ~(uint64_t)15) : lo;
    sl.pin.need((direct ? o_data : o_data + (size_t)bytes) + 16);
    uint8_t* pin = sl.pin.b();
    uint64_t* ro = reinterpret_cast<uint64_t*>(pin);
    uint8_t* dpin = sl.pin.dev;
    uint8_t* dblk = static_cast<uint8_t*>(device_view(d.block.get()));
    const uint8_t* drec = direct ? static_cast<const uint8_t*>(device_view(data + base)) : (dpin ? dpin + o_data : nullptr);
    if (!dpin || !dblk || !drec || (reinterpret_cast<uintptr_t>(drec) & 15u)) return false;
    for_ranges(n + 1, 8192, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) ro[i] = rec_off[i] - base;
    });
    if (!direct && bytes)
        for_ranges((size_t)bytes, size_t(1) << 16, [&](size_t x, size_t y) { copy_small(pin + o_data + x, data + lo + x, y - x); });
    sbe_decoded out{dblk,
                    dblk + d.o_fl,
                    reinterpret_cast<uint16_t*>(dblk + d.o_hdr),
                    reinterpret_cast<uint64_t*>(dblk + d.o_ts),
                    reinterpret_cast<uint32_t*>(dblk + d.o_off),
                    reinterpret_cast<uint32_t*>(dblk + d.o_len),
                    parse ? reinterpret_cast<uint64_t*>(dblk + d.o_seq) : nullptr};
    if (sbe_server* srv = c.server(n, true)) {  // inputs through the staging buffer, several workgroups
        if (sbe_serve_decode(srv, drec, reinterpret_cast<const uint64_t*>(dpin), n, mode, &out) == SBE_OK) return true;
        c.drop_server();
    }
    if (sbe_decode_batch_sized(drec, reinterpret_cast<const uint64_t*>(dpin), n, bytes, mode, &out, c.batch_stream()) !=
        SBE_OK) {
        c.abort_all();
        fail("sbe_decode_batch");
    }
    hip_check(hipStreamSynchronize(P.s_comp), "hipStreamSynchronize");
    return true;
}

std::shared_ptr<Descriptors> run_decode(const uint8_t* data, const uint64_t* rec_off, size_t n, uint32_t mode,
                                        const ChunkFn* on_chunk = nullptr) {
    auto d = std::make_shared<Descriptors>();
    d->n = n;
    if (n == 0) return d;
    Trace tr("decode");
    Ctx& c = ctx();
    Pipeline& P = c.pipe;
    const uint64_t base = rec_off[0], total = rec_off[n] - base;
    const size_t C = chunk_records(n, (size_t)total);
    const bool parse = mode == SBE_DEC_PARSE_MESSAGE;
    d->layout(C, parse);
    const size_t K = (n + C - 1) / C;
    P.serial = K == 1;
    const bool direct = page_locked(data + base, (size_t)total);  // no staging of the record bytes
    d->block = PinnedPool::get().take(K * d->chunk_bytes);
    uint8_t* hblk = static_cast<uint8_t*>(d->block.get());
    tr.lap(tr.plan);
    if (K == 1 && al16((n + 1) * 8) + (direct ? 0 : (size_t)total) <= zero_copy_max_bytes() &&
        decode_zero_copy(c, data, rec_off, n, mode, direct, *d)) {
        tr.lap(tr.sync);
        if (on_chunk) (*on_chunk)(*d, 0, n);
        tr.lap(tr.finish);
        tr.done(n, 0);
        return d;
    }
    PipeGuard guard(c);
    for (size_t k = 0; k < K; ++k) {
        const size_t a = k * C, m = std::min(n, a + C) - a;
        const uint64_t lo = rec_off[a], bytes = rec_off[a + m] - lo;
        const size_t o_data = al16((m + 1) * 8), in_bytes = o_data + bytes;
        Pipeline::Slot& sl = P.begin(k);
        tr.lap(tr.wait);
        sl.pin.need((direct ? o_data : in_bytes) + 16);
        uint8_t* pin = sl.pin.b();
        uint64_t* ro = reinterpret_cast<uint64_t*>(pin);
        // stage: the chunk's offsets rebased to 0 and (unless page-locked already) its bytes; on
        // the device the bytes start 16-B aligned after the offsets
        for_ranges(m + 1, 8192, [&](size_t x, size_t y) {
            for (size_t i = x; i < y; ++i) ro[i] = rec_off[a + i] - lo;
        });
        if (!direct)
            for_ranges((size_t)bytes, size_t(1) << 18, [&](size_t x, size_t y) {
                std::memcpy(pin + o_data + x, data + lo + x, y - x);
            });
        tr.lap(tr.stage);
        P.reserve(sl, in_bytes + 16, d->chunk_bytes);
        if (direct)
            P.copy_in(sl, (m + 1) * 8, data + lo, o_data, (size_t)bytes);
        else
            P.copy_in(sl, in_bytes);
        hipStream_t st = P.compute(sl);
        uint8_t* db = sl.d_out.b();
        sbe_decoded out{db,
                        db + d->o_fl,
                        reinterpret_cast<uint16_t*>(db + d->o_hdr),
                        reinterpret_cast<uint64_t*>(db + d->o_ts),
                        reinterpret_cast<uint32_t*>(db + d->o_off),
                        reinterpret_cast<uint32_t*>(db + d->o_len),
                        parse ? reinterpret_cast<uint64_t*>(db + d->o_seq) : nullptr};
        if (sbe_decode_batch_sized(sl.d_in.b() + o_data, reinterpret_cast<const uint64_t*>(sl.d_in.p), m, bytes, mode,
                                   &out, st) != SBE_OK)
            fail("sbe_decode_batch");
        st = P.copy_out(sl);
        hip_check(hipMemcpyAsync(hblk + k * d->chunk_bytes, db, d->chunk_bytes, hipMemcpyDeviceToHost, st), "D2H");
        P.end(sl);
        tr.lap(tr.enqueue);
        if (on_chunk && k > 0 && !P.serial) {  // chunk k-1, while chunk k is in flight
            hip_check(hipEventSynchronize(P.slot[(k - 1) % Pipeline::kSlots].out_done), "hipEventSynchronize");
            tr.lap(tr.sync);
            (*on_chunk)(*d, (k - 1) * C, std::min(n, k * C) - (k - 1) * C);
            tr.lap(tr.finish);
        }
    }
    c.sync_all();
    guard.release();
    tr.lap(tr.sync);
    if (on_chunk) {
        (*on_chunk)(*d, (K - 1) * C, n - (K - 1) * C);
        tr.lap(tr.finish);
    }
    tr.done(n, K);
    return d;
}

// Per-record output size of an encode (the plan the chunks are placed by; the device offsets are
// checked against it): overhead + Σ field lengths (PUBLISH_TOPIC: each mod 65536); a record with
// a field above 65534 B is an E109 and emits nothing.
struct EncodePlan {
    uint32_t overhead = 0;
    bool e109 = true;
    bool wrap16 = false;
    uint32_t layout = SBE_LAYOUT_TOPIC;  // tile shape of the kernels (planned serve encodes)
};

// Encode n records (nf strings, a u64 and a u32 each) through the chunk pipeline.  launch(...)
// issues one sbe_encode_*_batch call for a chunk on the given stream, or (server non-null: a small
// zero-copy batch) the synchronous sbe_serve_encode_* call (host_in: the inputs by their host
// addresses, the *_host form).
template <class Field, class U64, class U32, class Launch>
EncodedBatch run_encode(size_t n, int nf, Field&& field, U64&& u64, U32&& u32, EncodePlan plan, Launch&& launch) {
    EncodedBatch b;
    Trace tr("encode");
    if (n == 0) {
        b.offsets = HostBytesAccess::make<uint64_t>(1);
        b.offsets[0] = 0;
        return b;
    }
    Ctx& c = ctx();
    Pipeline& P = c.pipe;
    // per-record input (string) bytes and output bytes, prefixed, in one pass
    std::vector<uint64_t>& pin = c.pin;
    std::vector<uint64_t>& pout = c.pout;
    prefix2(n, pin, pout, [&](size_t i, uint64_t& in_b, uint64_t& out_b) {
        uint64_t si = 0, so = plan.overhead;
        bool e109 = false;
        for (int k = 0; k < nf; ++k) {
            const size_t L = field(i, k).size();
            si += L;
            so += plan.wrap16 ? (L & 0xFFFF) : L;
            e109 |= plan.e109 && L > SBE_VAR_MAX_LEN;
        }
        in_b = si;
        out_b = e109 ? 0 : so;
    });
    const size_t C = chunk_records(n, (size_t)(pin[n] + pout[n]) / 2);
    const size_t K = (n + C - 1) / C;
    P.serial = K == 1;
    {  // offsets | status | stream in one page-locked block (16-B aligned parts)
        const size_t o_st = al16((n + 1) * 8), o_by = o_st + al16(n);
        std::shared_ptr<void> blk = PinnedPool::get().take(o_by + (size_t)pout[n]);
        uint8_t* base = static_cast<uint8_t*>(blk.get());
        b.offsets = HostBytesAccess::view<uint64_t>(blk, base, n + 1);
        b.status = HostBytesAccess::view<uint8_t>(blk, base + o_st, n);
        b.bytes = HostBytesAccess::view<uint8_t>(blk, base + o_by, (size_t)pout[n]);
    }
    // staging layout of records [a, a + m): arena | u32 lengths [m][nf] | u64 [m] | u32 [m]
    struct Stage {
        size_t o_len, o_u64, o_u32, bytes;
    };
    auto stage_layout = [&](size_t a, size_t m) {
        const uint64_t in_bytes = pin[a + m] - pin[a];
        Stage s;
        s.o_len = al16((size_t)in_bytes);
        s.o_u64 = s.o_len + al16((size_t)m * 4 * nf);
        s.o_u32 = s.o_u64 + al16(m * 8);
        s.bytes = s.o_u32 + al16(m * 4);
        return s;
    };
    auto stage_fill = [&](uint8_t* p, const Stage& s, size_t a, size_t m) {
        const uint64_t in_lo = pin[a];
        uint32_t* lp = reinterpret_cast<uint32_t*>(p + s.o_len);
        uint64_t* up = reinterpret_cast<uint64_t*>(p + s.o_u64);
        uint32_t* wp = reinterpret_cast<uint32_t*>(p + s.o_u32);
        for_ranges(m, 1024, [&](size_t x, size_t y) {  // 256: 1 K-record encodes 5-9 us slower (wakes)
            for (size_t r = x; r < y; ++r) {
                const size_t i = a + r;
                uint8_t* at = p + (pin[i] - in_lo);
                for (int k2 = 0; k2 < nf; ++k2) {
                    const std::string_view f = field(i, k2);
                    copy_small(at, f.data(), f.size());
                    at += f.size();
                    lp[(size_t)nf * r + k2] = (uint32_t)f.size();
                }
                up[r] = u64(i);
                wp[r] = u32(i);
            }
        });
    };
    tr.lap(tr.plan);
    if (K == 1) {
        // zero-copy: the kernels read the page-locked staging buffer and write the stream, the
        // offsets and the status straight into the caller's page-locked result arrays
        const Stage s = stage_layout(0, n);
        Pipeline::Slot& sl = P.slot[0];
        if (s.bytes <= zero_copy_max_bytes()) {
            // one wave and inputs in its request slot (small batches), or several workgroups with
            // the tile sums of this plan after the staged inputs, or the batch launches
            sbe_server* srv = c.server(n);
            sbe_server* wsrv = srv ? nullptr : c.server(n, true);
            const size_t R = sbe_encode_tile_records(plan.layout), SB = 128 * R;
            const size_t tiles = (n + R - 1) / R, sbs = (n + SB - 1) / SB;
            const size_t o_sums = al16(s.bytes);
            sl.pin.need(wsrv ? o_sums + 16 * (tiles + sbs) : s.bytes);
            uint8_t* dp = sl.pin.dev;
            // offsets, status and stream share one block (above): one lookup for all three
            uint8_t* const hb = reinterpret_cast<uint8_t*>(b.offsets.data());
            uint8_t* const db = static_cast<uint8_t*>(device_view(hb));
            uint8_t* dbytes = db && pout[n] ? db + (b.bytes.data() - hb) : nullptr;
            uint64_t* doff = reinterpret_cast<uint64_t*>(db);
            uint8_t* dst = db ? db + (b.status.data() - hb) : nullptr;
            if (dp && doff && dst && (dbytes || pout[n] == 0)) {
                stage_fill(sl.pin.b(), s, 0, n);
                const uint64_t* tsums = nullptr;
                const uint64_t* bsums = nullptr;
                if (wsrv) {  // what sbe_enc_sums would compute, from the plan's prefix sums
                    uint64_t* ts = reinterpret_cast<uint64_t*>(sl.pin.b() + o_sums);
                    uint64_t* bs = ts + 2 * tiles;
                    for (size_t t = 0; t < tiles; ++t) {
                        const size_t r0 = t * R, b0 = (r0 / SB) * SB;
                        ts[2 * t] = pout[r0] - pout[b0];
                        ts[2 * t + 1] = pin[r0] - pin[b0];
                    }
                    for (size_t b = 0; b < sbs; ++b) {
                        const size_t r0 = b * SB, r1 = std::min(n, r0 + SB);
                        bs[2 * b] = pout[r1] - pout[r0];
                        bs[2 * b + 1] = pin[r1] - pin[r0];
                    }
                    tsums = reinterpret_cast<const uint64_t*>(dp + o_sums);
                    bsums = tsums + 2 * tiles;
                    srv = wsrv;
                }
                tr.lap(tr.stage);
                PipeGuard zguard(c);
                // a batch whose records all fail (E109) has no bytes: the kernels still want a
                // 16-B aligned output pointer, which they never write at capacity 0
                if (srv) {
                    c.d_ws.need(16);
                    // the single-wave serve takes the staged inputs by their host addresses (copied
                    // into its request slot when they fit, else read through their device addresses)
                    const uint8_t* ip = !wsrv && s.bytes <= SBE_SERVE_INLINE_BYTES ? sl.pin.b() : dp;
                    if (launch(srv, ip != dp, ip, reinterpret_cast<const uint32_t*>(ip + s.o_len),
                               reinterpret_cast<const uint64_t*>(ip + s.o_u64),
                               reinterpret_cast<const uint32_t*>(ip + s.o_u32), n, dbytes ? dbytes : c.d_ws.b(), pout[n],
                               doff, dst, c.d_ws.b(), 16, P.s_comp, tsums, bsums) != SBE_OK) {
                        c.drop_server();  // the batch kernels take this call and every later one
                        srv = nullptr;
                    }
                }
                if (!srv) {
                    const size_t ws_bytes = sbe_encode_workspace_size(n);
                    c.d_ws.need(ws_bytes);
                    hipStream_t st = c.batch_stream();
                    if (launch(nullptr, false, dp, reinterpret_cast<const uint32_t*>(dp + s.o_len),
                               reinterpret_cast<const uint64_t*>(dp + s.o_u64),
                               reinterpret_cast<const uint32_t*>(dp + s.o_u32), n, dbytes ? dbytes : c.d_ws.b(), pout[n],
                               doff, dst, c.d_ws.b(), ws_bytes, st, nullptr, nullptr) != SBE_OK)
                        fail("sbe_encode batch");
                    tr.lap(tr.enqueue);
                    hip_check(hipStreamSynchronize(st), "hipStreamSynchronize");
                }
                zguard.release();
                tr.lap(tr.sync);
                if (b.offsets[n] != pout[n]) throw std::logic_error("sbecodec: encoded batch size differs from its plan");
                tr.done(n, 0);
                return b;
            }
        }
    }
    // per-chunk device offsets (C + 1) and status (C), copied back beside each other
    const size_t meta_stride = al16((C + 1) * 8 + C);
    std::shared_ptr<void> meta = PinnedPool::get().take(K * meta_stride);
    uint8_t* hmeta = static_cast<uint8_t*>(meta.get());
    const size_t ws_bytes = sbe_encode_workspace_size(C);
    PipeGuard guard(c);
    for (size_t k = 0; k < K; ++k) {
        const size_t a = k * C, m = std::min(n, a + C) - a;
        const uint64_t out_lo = pout[a], out_bytes = pout[a + m] - out_lo;
        const Stage s = stage_layout(a, m);
        const size_t o_len = s.o_len, o_u64 = s.o_u64, o_u32 = s.o_u32, stage = s.bytes;
        Pipeline::Slot& sl = P.begin(k);
        tr.lap(tr.wait);
        sl.pin.need(stage);
        stage_fill(sl.pin.b(), s, a, m);
        tr.lap(tr.stage);
        // device: out bytes | out_off [m+1] | status [m] | workspace
        const size_t d_off = al16((size_t)out_bytes), d_ws = d_off + meta_stride;
        P.reserve(sl, stage, d_ws + ws_bytes);
        P.copy_in(sl, stage);
        hipStream_t st = P.compute(sl);
        const uint8_t* di = sl.d_in.b();
        uint8_t* dout = sl.d_out.b();
        if (launch(nullptr, false, di, reinterpret_cast<const uint32_t*>(di + o_len),
                   reinterpret_cast<const uint64_t*>(di + o_u64), reinterpret_cast<const uint32_t*>(di + o_u32), m, dout,
                   out_bytes, reinterpret_cast<uint64_t*>(dout + d_off), dout + d_off + (m + 1) * 8, dout + d_ws, ws_bytes,
                   st, nullptr, nullptr) != SBE_OK)
            fail("sbe_encode batch");
        st = P.copy_out(sl);
        if (out_bytes) hip_check(hipMemcpyAsync(b.bytes.data() + out_lo, dout, out_bytes, hipMemcpyDeviceToHost, st), "D2H");
        hip_check(hipMemcpyAsync(hmeta + k * meta_stride, dout + d_off, (m + 1) * 8 + m, hipMemcpyDeviceToHost, st), "D2H");
        P.end(sl);
        tr.lap(tr.enqueue);
    }
    c.sync_all();
    guard.release();
    tr.lap(tr.sync);
    for (size_t k = 0; k < K; ++k) {
        const size_t a = k * C, m = std::min(n, a + C) - a;
        const uint64_t* off = reinterpret_cast<const uint64_t*>(hmeta + k * meta_stride);
        if (off[m] != pout[a + m] - pout[a])
            throw std::logic_error("sbecodec: encoded chunk size differs from its plan");
    }
    for_ranges(n, 16384, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) {
            const size_t k = i / C, j = i - k * C, m = std::min(n, k * C + C) - k * C;
            const uint8_t* mk = hmeta + k * meta_stride;
            b.offsets[i] = pout[k * C] + reinterpret_cast<const uint64_t*>(mk)[j];
            b.status[i] = mk[(m + 1) * 8 + j];
        }
    });
    b.offsets[n] = pout[n];
    tr.lap(tr.finish);
    tr.done(n, K);
    return b;
}

inline int64_t rdi64(const uint8_t* p) {
    uint64_t v = 0;
    for (int i = 7; i >= 0; --i) v = (v << 8) | p[i];
    return (int64_t)v;
}
inline int32_t rdi32(const uint8_t* p) { return (int32_t)((uint32_t)p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24)); }
inline uint16_t rdu16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// r := the ParseResult of record i, every field rewritten; the strings are assigned in place, so a
// reused ParseResult keeps its buffers (parse_batch into a caller's vector allocates nothing once
// the strings have grown to the records' sizes)
void materialize_into(ParseResult& r, const uint8_t* rec, const Descriptors& d, size_t i) {
    r.success = false;
    r.timestamp = 0;
    r.sequence_number = 0;
    r.template_id = r.schema_id = r.version = r.block_length = 0;
    r.correlation_id = r.session_id = r.leadership_term_id = 0;
    r.leader_member_id = r.event_code = 0;
    r.sequence_key_present = false;
    const uint8_t st = d.status(i), fl = d.flags(i);
    const uint16_t* h = d.hdr(i);
    const uint32_t* off = d.off(i);
    const uint32_t* len = d.len(i);
    struct View {  // record bytes [off[k], off[k] + len[k]), assigned into a string in place
        const char* p;
        uint32_t n;
    };
    auto view = [&](int k) { return View{reinterpret_cast<const char*>(rec) + off[k], len[k]}; };
    // strings the status's branch writes (the others are cleared after it): resized only when the
    // length changes, so a reused ParseResult of the same shape is overwritten in place
    enum : unsigned { kType = 2, kId = 4, kPay = 8, kHdr = 16 };
    unsigned written = 0;
    auto set = [&](std::string& s, View v, unsigned which) {
        if (s.size() != v.n) s.resize(v.n);
        copy_small(s.data(), v.p, v.n);
        written |= which;
    };
    auto put = [&](std::string& s, std::string&& v, unsigned which) {
        s = std::move(v);
        written |= which;
    };
    auto take_hdr = [&] {
        r.block_length = h[0];
        r.template_id = h[1];
        r.schema_id = h[2];
        r.version = h[3];
    };
    const uint32_t param = off[0];
    switch (st) {
        case SBE_ST_TM:  // src/sbe_encoder.cpp:1021-1135
            r.success = true;
            set(r.message_type, view(1), kType);
            set(r.message_id, view(2), kId);
            set(r.payload, view(3), kPay);
            set(r.headers, view(4), kHdr);
            r.timestamp = (int64_t)d.ts(i);
            r.sequence_key_present = (fl & SBE_FL_SEQ_KEY) != 0;
            r.sequence_number = d.seq(i);  // src/sbe_encoder.cpp:1031-1125
            take_hdr();
            break;
        case SBE_ST_ACK:  // src/sbe_encoder.cpp:916-941
            r.success = true;
            set(r.message_type, View{"Acknowledgment", 14}, kType);
            r.timestamp = (int64_t)d.ts(i);
            if (fl & SBE_FL_ID_DEFAULT)
                put(r.message_id, "ack_" + std::to_string(d.ts(i)), kId);
            else
                set(r.message_id, view(0), kId);
            if (fl & SBE_FL_PAYLOAD_DEFAULT)
                set(r.payload, View{"SUCCESS", 7}, kPay);
            else
                set(r.payload, view(1), kPay);
            set(r.headers, view(2), kHdr);
            take_hdr();
            break;
        case SBE_ST_SESSION_EVENT:  // src/sbe_encoder.cpp:629-644 (SessionEvent layout sbe_messages.hpp:39-50)
            r.success = true;
            set(r.message_type, View{"SessionEvent", 12}, kType);
            r.correlation_id = rdi64(rec + 8);
            r.session_id = rdi64(rec + 16);
            r.leadership_term_id = rdi64(rec + 24);
            r.leader_member_id = rdi32(rec + 32);
            r.event_code = rdi32(rec + 36);
            set(r.payload, view(3), kPay);
            r.timestamp = 0;
            take_hdr();
            break;
        case SBE_ST_ERR_NULL_EMPTY: r.error_message = "Null or empty data"; break;
        case SBE_ST_ERR_HEADER: r.error_message = "Failed to decode message header"; break;
        case SBE_ST_ERR_UNKNOWN_TYPE:
            take_hdr();
            r.error_message = "Unknown message type: template=" + std::to_string(r.template_id) +
                              ", schema=" + std::to_string(r.schema_id);
            break;
        case SBE_ST_ERR_SESSION_EVENT: r.error_message = "Failed to decode SessionEvent"; break;
        case SBE_ST_ERR_SESSION_SHORT: r.error_message = "Session message too short to contain embedded message"; break;
        case SBE_ST_ERR_EMBEDDED_SHORT: r.error_message = "Embedded message too short"; break;
        case SBE_ST_ERR_EMBEDDED_TEMPLATE:
            r.error_message = "Unknown embedded message template_id: " + std::to_string(param);
            break;
        case SBE_ST_ERR_EMBEDDED_SCHEMA:
            r.error_message = "Unknown embedded message schema_id: " + std::to_string(param);
            break;
        case SBE_ST_ERR_DIRECT_TEMPLATE:
            r.error_message = "Unknown direct message template_id: " + std::to_string(param);
            break;
        case SBE_ST_ERR_TM_E100: r.error_message = "SBE TopicMessage decoding failed: buffer too short [E100]"; break;
        case SBE_ST_ERR_ACK_SHORT:
            r.error_message = "Buffer too short for Acknowledgment message. Need at least 16 bytes, got " +
                              std::to_string(param);
            break;
        default: throw std::runtime_error("sbecodec: unexpected parse status");
    }
    if (st < SBE_ST_ERR_NULL_EMPTY) r.error_message.clear();  // every error branch above sets it
    if (!(written & kType)) r.message_type.clear();
    if (!(written & kId)) r.message_id.clear();
    if (!(written & kPay)) r.payload.clear();
    if (!(written & kHdr)) r.headers.clear();
}

ParseResult materialize(const uint8_t* rec, const Descriptors& d, size_t i) {
    ParseResult r;
    materialize_into(r, rec, d, i);
    return r;
}

const char* kE109[5] = {"topicLength too long for length type [E109]", "messageTypeLength too long for length type [E109]",
                        "uuidLength too long for length type [E109]", "payloadLength too long for length type [E109]",
                        "headersLength too long for length type [E109]"};

std::string_view tm_field(const TopicMessageFields& m, int k) {
    switch (k) {
        case 0: return m.topic;
        case 1: return m.message_type;
        case 2: return m.uuid;
        case 3: return m.payload;
        default: return m.headers;
    }
}

uint64_t clock_ms() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::milliseconds>(
               std::chrono::system_clock::now().time_since_epoch())
        .count();
}
uint64_t clock_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::high_resolution_clock::now().time_since_epoch())
        .count();
}
uint64_t now_nanos_sys() {  // include/aeron_cluster/protocol.hpp:31-34
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::system_clock::now().time_since_epoch())
        .count();
}

EncodedBatch encode_tm(const std::vector<TopicMessageFields>& msgs, EncodeLength length, bool session, int64_t term,
                       int64_t sess, uint64_t ts_default) {
    const uint32_t flags = length == EncodeLength::Reference ? SBE_ENC_REF_TRUNCATE8
                         : length == EncodeLength::Publish   ? SBE_ENC_PUBLISH_TOPIC
                                                             : 0u;
    EncodePlan plan;
    plan.overhead = (length == EncodeLength::Reference ? SBE_TM_REF_OVERHEAD : SBE_TM_WIRE_OVERHEAD) +
                    (session ? SBE_SESSION_HDR_LEN : 0u);
    plan.e109 = length != EncodeLength::Publish;
    plan.wrap16 = length == EncodeLength::Publish;
    plan.layout = session ? SBE_LAYOUT_SESSION : SBE_LAYOUT_TOPIC;
    return run_encode(
        msgs.size(), 5, [&](size_t i, int k) { return tm_field(msgs[i], k); },
        [&](size_t i) { return (uint64_t)msgs[i].timestamp; }, [](size_t) { return 0u; }, plan,
        [&](sbe_server* srv, bool host_in, const uint8_t* arena, const uint32_t* len, const uint64_t* ts,
            const uint32_t*, size_t m, uint8_t* out, uint64_t cap, uint64_t* off, uint8_t* st, void* ws, size_t wsb,
            hipStream_t s, const uint64_t* tsums, const uint64_t* bsums) {
            sbe_tm_batch in{arena, nullptr, len, ts};
            int rc;
            if (srv && tsums)
                rc = session ? sbe_serve_encode_session_planned(srv, &in, m, ts_default, flags, term, sess, out, cap, off,
                                                                st, tsums, bsums)
                             : sbe_serve_encode_topic_planned(srv, &in, m, ts_default, flags, out, cap, off, st, tsums,
                                                              bsums);
            else if (srv && host_in)
                rc = session ? sbe_serve_encode_session_host(srv, &in, m, ts_default, flags, term, sess, out, cap, off, st)
                             : sbe_serve_encode_topic_host(srv, &in, m, ts_default, flags, out, cap, off, st);
            else if (srv)
                rc = session ? sbe_serve_encode_session(srv, &in, m, ts_default, flags, term, sess, out, cap, off, st)
                             : sbe_serve_encode_topic(srv, &in, m, ts_default, flags, out, cap, off, st);
            else
                rc = session ? sbe_encode_session_batch(&in, m, ts_default, flags, term, sess, out, cap, off, st, ws,
                                                        wsb, s)
                             : sbe_encode_topic_batch(&in, m, ts_default, flags, out, cap, off, st, ws, wsb, s);
            return rc;
        });
}

// DEBUG_LOG of the reference (include/aeron_cluster/debug_utils.hpp:11-28, 71): on stdout when
// AERON_CLUSTER_DEBUG=1
bool debug_enabled() {
    static const bool on = [] {
        const char* e = std::getenv("AERON_CLUSTER_DEBUG");
        return e && std::string(e) == "1";
    }();
    return on;
}
template <class... A>
void debug_log(const A&... a) {
    if (!debug_enabled()) return;
    std::cout << "[DEBUG] ";
    (std::cout << ... << a);
    std::cout << std::endl;
}

}  // namespace

// ======================================================================================
// SBEUtils (src/sbe_encoder.cpp:328-485) and ParseResult (sbe_messages.hpp:340-411)
// ======================================================================================
namespace SBEUtils {

void print_hex_dump(const std::uint8_t* data, std::size_t length, const std::string& prefix, std::size_t max_bytes) {
    if (!data || length == 0) return;
    const size_t shown = max_bytes > 0 ? std::min(length, max_bytes) : length;
    for (size_t row = 0; row < shown; row += 16) {
        std::cout << prefix << std::setfill('0') << std::setw(4) << std::hex << row << ": ";
        for (size_t j = 0; j < 16; ++j) {
            if (row + j < shown)
                std::cout << std::setfill('0') << std::setw(2) << std::hex << static_cast<unsigned>(data[row + j]) << " ";
            else
                std::cout << "   ";
            if (j == 7) std::cout << " ";
        }
        std::cout << " |";
        for (size_t j = 0; j < 16 && row + j < shown; ++j) {
            const char ch = static_cast<char>(data[row + j]);
            std::cout << ((ch >= 32 && ch <= 126) ? ch : '.');
        }
        std::cout << "|" << std::dec << std::endl;
    }
    if (max_bytes > 0 && length > max_bytes) std::cout << prefix << "... (" << (length - max_bytes) << " more bytes)" << std::endl;
}

std::string get_session_event_code_string(std::int32_t code) {
    switch (code) {
        case SBEConstants::SESSION_EVENT_OK: return "OK";
        case SBEConstants::SESSION_EVENT_ERROR: return "ERROR";
        case SBEConstants::SESSION_EVENT_AUTHENTICATION_REJECTED: return "AUTHENTICATION_REJECTED";
        case SBEConstants::SESSION_EVENT_REDIRECT: return "REDIRECT";
        case SBEConstants::SESSION_EVENT_CLOSED: return "CLOSED";
        default: return "UNKNOWN(" + std::to_string(code) + ")";
    }
}

std::string get_message_type_name(std::uint16_t template_id, std::uint16_t schema_id) {
    if (schema_id == SBEConstants::CLUSTER_SCHEMA_ID) {
        if (template_id == SBEConstants::SESSION_CONNECT_TEMPLATE_ID) return "SessionConnectRequest";
        if (template_id == SBEConstants::SESSION_EVENT_TEMPLATE_ID) return "SessionEvent";
        return "UnknownClusterMessage(" + std::to_string(template_id) + ")";
    }
    if (schema_id == SBEConstants::TOPIC_SCHEMA_ID) {
        if (template_id == SBEConstants::TOPIC_MESSAGE_TEMPLATE_ID) return "TopicMessage";
        if (template_id == SBEConstants::ACKNOWLEDGMENT_TEMPLATE_ID) return "Acknowledgment";
        return "UnknownTopicMessage(" + std::to_string(template_id) + ")";
    }
    return "UnknownSchema(" + std::to_string(schema_id) + "," + std::to_string(template_id) + ")";
}

bool is_valid_correlation_id(std::int64_t correlation_id) { return correlation_id > 0; }

std::int64_t generate_correlation_id() {
    return (std::int64_t)std::chrono::high_resolution_clock::now().time_since_epoch().count() & 0x7FFFFFFFFFFFFFFFLL;
}

std::string format_timestamp(std::int64_t timestamp) {
    const std::time_t secs = std::chrono::system_clock::to_time_t(
        std::chrono::time_point<std::chrono::system_clock>(std::chrono::nanoseconds(timestamp)));
    std::stringstream ss;
    ss << std::put_time(std::gmtime(&secs), "%Y-%m-%d %H:%M:%S UTC");
    ss << "." << std::setfill('0') << std::setw(9) << (timestamp % 1000000000);
    return ss.str();
}

bool is_valid_sbe_message(const std::uint8_t* data, std::size_t length) {
    if (!data || length < SBEConstants::SBE_HEADER_LENGTH) return false;
    const uint16_t blk = rdu16(data), schema = rdu16(data + 4);
    if (blk == 0 || blk > 10000) return false;
    if (length < SBEConstants::SBE_HEADER_LENGTH + blk) return false;
    return schema == SBEConstants::CLUSTER_SCHEMA_ID || schema == SBEConstants::TOPIC_SCHEMA_ID;
}

std::vector<std::string> extract_readable_strings(const std::uint8_t* data, std::size_t length, std::size_t min_length) {
    std::vector<std::string> out;
    if (!data || length == 0) return out;
    size_t start = 0;
    for (size_t i = 0; i <= length; ++i) {
        const bool printable = i < length && data[i] >= 32 && data[i] <= 126;
        if (printable) continue;
        if (i - start >= min_length) out.emplace_back(reinterpret_cast<const char*>(data) + start, i - start);
        start = i + 1;
    }
    return out;
}

}  // namespace SBEUtils

bool ParseResult::is_topic_message() const {
    if (template_id == SBEConstants::TOPIC_MESSAGE_TEMPLATE_ID && schema_id == SBEConstants::TOPIC_SCHEMA_ID) return true;
    if (schema_id == SBEConstants::CLUSTER_SCHEMA_ID && template_id == SBEConstants::TOPIC_MESSAGE_TEMPLATE_ID) return true;
    if (schema_id == SBEConstants::TOPIC_SCHEMA_ID && template_id == SBEConstants::SESSION_EVENT_TEMPLATE_ID) return true;
    if (!message_type.empty() &&
        (message_type.find("ORDER") != std::string::npos || message_type.find("TopicMessage") != std::string::npos ||
         message_type.find("CREATE_ORDER") != std::string::npos || message_type.find("UPDATE_ORDER") != std::string::npos))
        return true;
    return false;
}

bool ParseResult::is_order_message() const {
    if (!is_topic_message()) return false;
    // every keyword of the reference's type list contains "ORDER" (sbe_messages.hpp:386-391)
    if (!message_type.empty() && message_type.find("ORDER") != std::string::npos) return true;
    if (payload.empty()) return false;
    for (const char* k : {"order_details", "token_pair", "quantity", "side", "client_order_id"})
        if (payload.find(k) != std::string::npos) return true;
    return false;
}

std::string ParseResult::get_description() const {
    std::stringstream ss;
    if (success) {
        ss << SBEUtils::get_message_type_name(template_id, schema_id);
        if (is_session_event())
            ss << " (code: " << SBEUtils::get_session_event_code_string(event_code) << ")";
        else if (!message_type.empty())
            ss << " (type: " << message_type << ")";
        if (!message_id.empty()) ss << " [ID: " << message_id.substr(0, 8) << "...]";
    } else {
        ss << "Parse Error: " << error_message;
    }
    return ss.str();
}

// ======================================================================================
// SBEDecoder (src/sbe_encoder.cpp:174-323): one-record struct readers, host code (see the header)
// ======================================================================================
namespace {
// SBEDecoder::extract_variable_string (:285-318): a u32 length prefix at offset, the string after
// it; 0 (output untouched) when the prefix or the string does not fit or the length is over 10 MiB.
// The reference checks the length against `remaining - 4` whatever the offset (:302), so for a
// field after the first one a corrupt length can make it read up to `offset` bytes past the
// record (undefined behaviour on network input).  Here the string must end inside the record:
// identical results for every record the reference reads in bounds, a refusal for the others.
size_t extract_variable_string(const uint8_t* data, size_t offset, size_t remaining, std::string& output) {
    if (offset + sizeof(uint32_t) > remaining) {
        debug_log("[ERROR] Not enough data for length prefix at offset ", offset, ", remaining: ", remaining);
        return 0;
    }
    uint32_t length;
    std::memcpy(&length, data + offset, sizeof(uint32_t));
    debug_log("[DEBUG] Extracting string at offset ", offset, ", length prefix: ", length, ", remaining: ", remaining);
    offset += sizeof(uint32_t);
    if (length > remaining - offset || length > 10u * 1024u * 1024u) {
        debug_log("[ERROR] Invalid string length: ", length, ", remaining data: ", (remaining - sizeof(uint32_t)));
        return 0;
    }
    if (length > 0) {
        output.assign(reinterpret_cast<const char*>(data + offset), length);
        offset += length;
        debug_log("[DEBUG] Extracted string: \"", output, "\"");
    } else {
        output.clear();
        debug_log("[DEBUG] Extracted empty string");
    }
    return offset;
}
}  // namespace

bool SBEDecoder::decode_message_header(const std::uint8_t* data, std::size_t length, MessageHeader& header) {
    if (!data || length < sizeof(MessageHeader)) return false;
    std::memcpy(&header, data, sizeof(MessageHeader));
    return true;
}

bool SBEDecoder::decode_session_event(const std::uint8_t* data, std::size_t length, SessionEvent& event,
                                      std::string& detail) {
    if (!data || length < sizeof(MessageHeader) + SessionEvent::sbe_block_length()) return false;
    if (debug_enabled()) {  // the reference's raw-data diagnostics (:189-214)
        debug_log("Raw data analysis (", length, " bytes)");
        debug_log("Hex dump: ");
        for (size_t i = 0; i < length && i < 64; ++i) {
            debug_log("0x", static_cast<unsigned>(data[i]), " ");
            if ((i + 1) % 16 == 0) debug_log("\n          ");
        }
        debug_log("Readable content: ");
        std::string readable;
        for (size_t i = 0; i < length && i < 256; ++i) {
            const char ch = static_cast<char>(data[i]);
            if (ch >= 32 && ch <= 126) {
                readable += ch;
            } else if (!readable.empty()) {
                if (readable.length() >= 3) debug_log("\"", readable, "\" ");
                readable.clear();
            }
        }
        if (readable.length() >= 3) debug_log("\"", readable, "\"");
    }
    MessageHeader header;
    if (!decode_message_header(data, length, header)) return false;
    if (!(header.template_id == SessionEvent::sbe_template_id() && header.schema_id == SessionEvent::sbe_schema_id()))
        return false;
    std::memcpy(&event, data + sizeof(MessageHeader), SessionEvent::sbe_block_length());
    const size_t remaining = length - sizeof(MessageHeader) - SessionEvent::sbe_block_length();
    if (remaining > 0)
        extract_variable_string(data + sizeof(MessageHeader) + SessionEvent::sbe_block_length(), 0, remaining, detail);
    return true;
}

bool SBEDecoder::decode_acknowledgment(const std::uint8_t* data, std::size_t length, std::string& message_id,
                                       std::string& status, std::string& error, std::int64_t& timestamp) {
    constexpr size_t kAckBlock = 8;  // Acknowledgment::sbe_block_length() (sbe_messages.hpp:106-118)
    if (!data || length < sizeof(MessageHeader) + kAckBlock) return false;
    MessageHeader header;
    if (!decode_message_header(data, length, header)) return false;
    if (!(header.template_id == SBEConstants::ACKNOWLEDGMENT_TEMPLATE_ID && header.schema_id == SBEConstants::TOPIC_SCHEMA_ID))
        return false;
    const uint8_t* ptr = data + sizeof(MessageHeader);
    std::memcpy(&timestamp, ptr, sizeof(int64_t));
    ptr += kAckBlock;
    const size_t remaining = length - sizeof(MessageHeader) - kAckBlock;
    size_t offset = extract_variable_string(ptr, 0, remaining, message_id);
    if (offset == 0) return false;
    offset = extract_variable_string(ptr, offset, remaining, status);
    if (offset == 0) return false;
    if (offset < remaining) extract_variable_string(ptr, offset, remaining, error);
    return true;
}

std::int64_t SBEEncoder::get_current_timestamp() {
    return (std::int64_t)std::chrono::high_resolution_clock::now().time_since_epoch().count();
}

void quiesce() { ctx().quiesce(); }

bool gpu_codec_available() { return sbe_device_ready() == 1; }
unsigned host_threads() { return Workers::get().size(); }

void host_register(const void* p, std::size_t len) {
    hip_check(hipHostRegister(const_cast<void*>(p), len, hipHostRegisterDefault), "hipHostRegister");
    PinnedRegistry::get().add(p, len);
}
void host_unregister(const void* p) {
    PinnedRegistry::get().remove(p);
    hip_check(hipHostUnregister(const_cast<void*>(p)), "hipHostUnregister");
}

// ======================================================================================
// encode
// ======================================================================================
EncodedBatch SBEEncoder::encode_topic_batch(const std::vector<TopicMessageFields>& msgs, EncodeLength length) {
    Trace tr("encode_topic_batch");
    // timestamp 0 → the clock the reference reads (src/sbe_encoder.cpp:134-138)
    EncodedBatch b = encode_tm(msgs, length, false, 0, 0, clock_ms());
    tr.done(msgs.size(), 0);
    return b;
}

std::vector<std::uint8_t> SBEEncoder::encode_topic_message(const std::string& topic, const std::string& message_type,
                                                           const std::string& uuid, const std::string& payload,
                                                           const std::string& headers, std::int64_t timestamp) {
    TopicMessageFields f{topic, message_type, uuid, payload, headers, timestamp};
    EncodedBatch b = encode_topic_batch({f}, EncodeLength::Reference);
    const uint8_t st = b.status[0];
    if (st >= SBE_ENC_E109_TOPIC && st <= SBE_ENC_E109_HEADERS) throw std::runtime_error(kE109[st - 1]);
    if (st != SBE_ENC_OK) throw std::runtime_error("sbecodec: encode failed");
    return b.bytes.to_vector();
}

EncodedBatch SessionFrameEncoder::encode_batch(const std::vector<TopicMessageFields>& msgs, EncodeLength length) const {
    // create_topic_message stamps high_resolution_clock nanoseconds (src/session_manager.cpp:1075-1076)
    return encode_tm(msgs, length, true, leadership_term_id_, cluster_session_id_, clock_ns());
}

std::vector<std::uint8_t> SessionFrameEncoder::create_combined_message(const std::string& topic,
                                                                       const std::string& message_type,
                                                                       const std::string& message_id,
                                                                       const std::string& payload,
                                                                       const std::string& headers) const {
    TopicMessageFields f{topic, message_type, message_id, payload, headers, 0};
    EncodedBatch b = encode_batch({f}, EncodeLength::Reference);
    const uint8_t st = b.status[0];
    if (st >= SBE_ENC_E109_TOPIC && st <= SBE_ENC_E109_HEADERS) throw std::runtime_error(kE109[st - 1]);
    if (st != SBE_ENC_OK) throw std::runtime_error("sbecodec: encode failed");
    return b.bytes.to_vector();
}

std::vector<std::string> TopicPublisher::publish_topic_batch(const std::vector<TopicMessageFields>& msgs) {
    const size_t n = msgs.size();
    std::vector<std::string> uuids(n);
    std::vector<TopicMessageFields> f(msgs);
    for (size_t i = 0; i < n; ++i) {
        uuids[i] = std::string("pub_") + std::to_string(now_nanos_sys());  // src/cluster_client.cpp:1818
        f[i].uuid = uuids[i];
        if (f[i].headers.empty()) f[i].headers = "{}";                     // :1821
        f[i].timestamp = (int64_t)now_nanos_sys();                         // :1845
    }
    EncodedBatch b = encode_tm(f, EncodeLength::Publish, false, 0, 0, now_nanos_sys());
    std::vector<std::string> sent;
    std::vector<uint64_t> sent_ts;
    for (size_t i = 0; i < n; ++i) {
        const bool ok = offer_(b.bytes.data() + b.offsets[i], b.offsets[i + 1] - b.offsets[i]);
        if (ok && correlator_) {  // remember_outgoing(uuid, ts), src/cluster_client.cpp:1860-1861
            sent.push_back(uuids[i]);
            sent_ts.push_back((uint64_t)f[i].timestamp);
        }
    }
    if (!sent.empty()) correlator_->remember_batch(sent, sent_ts);
    return uuids;
}

std::string TopicPublisher::publish_topic(std::string_view topic, std::string_view message_type,
                                          std::string_view json_payload, std::string_view headers_json) {
    TopicMessageFields m{topic, message_type, {}, json_payload, headers_json, 0};
    return publish_topic_batch({m})[0];
}

std::uint32_t CommitManager::topic_to_id(const std::string& topic) {
    if (topic == "order_request_topic") return 1;
    if (topic == "order_notification_topic") return 2;
    if (topic == "orders") return 3;
    if (topic == "order_status_request_topic") return 4;
    return 0;
}

EncodedBatch CommitManager::build_commit_offset_batch(const std::vector<CommitOffset>& offsets) const {
    std::vector<uint32_t> ids(offsets.size());
    for (size_t i = 0; i < offsets.size(); ++i) {
        ids[i] = topic_to_id(offsets[i].topic);
        if (ids[i] == 0)
            throw std::runtime_error("sbecodec: commit offset for unknown topic '" + offsets[i].topic +
                                     "' needs the JSON TopicMessage fallback (build_commit_offset_fallback)");
    }
    EncodePlan plan;
    plan.overhead = SBE_LITE_OVERHEAD(2);
    plan.layout = SBE_LAYOUT_LITE;
    return run_encode(
        offsets.size(), 2,
        [&](size_t i, int k) { return std::string_view(k == 0 ? offsets[i].message_id : offsets[i].message_identifier); },
        [&](size_t i) { return offsets[i].sequence_number; }, [&](size_t i) { return ids[i]; }, plan,
        [&](sbe_server* srv, bool host_in, const uint8_t* arena, const uint32_t* len, const uint64_t* seq,
            const uint32_t* tid, size_t m, uint8_t* out, uint64_t cap, uint64_t* off, uint8_t* st, void* ws, size_t wsb,
            hipStream_t s, const uint64_t* tsums, const uint64_t* bsums) {
            sbe_lite_batch in{arena, nullptr, len, tid, seq};
            const int rc =
                srv && tsums ? sbe_serve_encode_lite_planned(srv, &in, m, SBE_COMMIT_OFFSET_LITE_TEMPLATE_ID, out, cap,
                                                             off, st, tsums, bsums)
                : srv && host_in ? sbe_serve_encode_lite_host(srv, &in, m, SBE_COMMIT_OFFSET_LITE_TEMPLATE_ID, out, cap, off, st)
                : srv          ? sbe_serve_encode_lite(srv, &in, m, SBE_COMMIT_OFFSET_LITE_TEMPLATE_ID, out, cap, off, st)
                               : sbe_encode_lite_batch(&in, m, SBE_COMMIT_OFFSET_LITE_TEMPLATE_ID, out, cap, off, st, ws,
                                                       wsb, s);
            return rc;
        });
}

std::vector<std::uint8_t> CommitManager::build_commit_offset_message(const std::string& topic,
                                                                     const std::string& client_id,
                                                                     const CommitOffset& offset) const {
    (void)topic;  // the reference keys the template on offset.topic (src/commit_manager.cpp:110)
    (void)client_id;
    EncodedBatch b = build_commit_offset_batch({offset});
    static const char* kLiteE109[2] = {"messageIdLength too long for length type [E109]",
                                       "messageIdentifierLength too long for length type [E109]"};
    const uint8_t st = b.status[0];
    if (st == 1 || st == 2) throw std::runtime_error(kLiteE109[st - 1]);
    if (st != SBE_ENC_OK) throw std::runtime_error("sbecodec: encode failed");
    return b.bytes.to_vector();
}

namespace {
// jsoncpp valueToQuotedStringN(s, emitUTF8 = false), utf8ToCodepoint included (json_writer.cpp):
// what csrc/order_json.hpp's oj::quoted writes on the device.
void json_quote(std::string& out, std::string_view s) {
    auto hex4 = [&](uint32_t v) {
        static const char hx[] = "0123456789abcdef";
        out += "\\u";
        for (int sh = 12; sh >= 0; sh -= 4) out += hx[(v >> sh) & 15];
    };
    out += '"';
    for (size_t i = 0; i < s.size();) {
        const uint32_t c = (uint8_t)s[i];
        const size_t left = s.size() - i;
        auto at = [&](size_t k) { return (uint32_t)(uint8_t)s[i + k]; };
        switch (c) {
            case '"': out += "\\\""; ++i; continue;
            case '\\': out += "\\\\"; ++i; continue;
            case '\b': out += "\\b"; ++i; continue;
            case '\f': out += "\\f"; ++i; continue;
            case '\n': out += "\\n"; ++i; continue;
            case '\r': out += "\\r"; ++i; continue;
            case '\t': out += "\\t"; ++i; continue;
            default: break;
        }
        if (c >= 0x20 && c < 0x80) {
            out += (char)c;
            ++i;
            continue;
        }
        uint32_t cp = 0xFFFD;
        size_t used = 1;
        if (c < 0x20) {
            cp = c;
        } else if (c < 0xE0) {
            if (left >= 2) {
                cp = ((c & 0x1F) << 6) | (at(1) & 0x3F);
                used = 2;
                if (cp < 0x80) cp = 0xFFFD;
            }
        } else if (c < 0xF0) {
            if (left >= 3) {
                cp = ((c & 0x0F) << 12) | ((at(1) & 0x3F) << 6) | (at(2) & 0x3F);
                used = 3;
                if ((cp >= 0xD800 && cp <= 0xDFFF) || cp < 0x800) cp = 0xFFFD;
            }
        } else if (c < 0xF8) {
            if (left >= 4) {
                cp = ((c & 0x07) << 18) | ((at(1) & 0x3F) << 12) | ((at(2) & 0x3F) << 6) | (at(3) & 0x3F);
                used = 4;
                if (cp < 0x10000) cp = 0xFFFD;
            }
        }
        i += used;
        if (cp < 0x10000) {
            hex4(cp);
        } else {
            cp -= 0x10000;
            hex4(0xD800 + ((cp >> 10) & 0x3FF));
            hex4(0xDC00 + (cp & 0x3FF));
        }
    }
    out += '"';
}
}  // namespace

std::string CommitManager::serialize_commit_offset(const CommitOffset& offset) {
    std::string t = "{\"action\":\"COMMIT_OFFSET\",\"messageIdentifier\":";
    json_quote(t, offset.message_identifier);
    t += ",\"message_id\":";
    json_quote(t, offset.message_id);
    t += ",\"sequence_number\":" + std::to_string(offset.sequence_number);
    t += ",\"timestamp_nanos\":" + std::to_string(offset.timestamp_nanos);
    t += ",\"topic\":";
    json_quote(t, offset.topic);
    t += '}';
    return t;
}

std::vector<std::uint8_t> CommitManager::build_commit_offset_fallback(const std::string& client_id,
                                                                      const CommitOffset& offset,
                                                                      const ClockFn& clock) const {
    auto now = [&] { return clock ? clock() : now_nanos_sys(); };
    const std::string text = serialize_commit_offset(offset);
    std::vector<std::uint8_t> buf;
    buf.reserve(SBE_CE_FALLBACK_REC_MAX);
    auto put16 = [&](uint32_t v) {
        buf.push_back((uint8_t)v);
        buf.push_back((uint8_t)(v >> 8));
    };
    auto put64 = [&](uint64_t v) {
        for (int b = 0; b < 8; ++b) buf.push_back((uint8_t)(v >> (8 * b)));
    };
    // put*(const char*, std::uint16_t): the length mod 65536 and that many leading bytes; the
    // flyweight's limit is 1040 absolute (wrapForEncode(buf, 8, 1048 - 8))
    auto put_var = [&](std::string_view v) {
        const size_t len = v.size() & 0xffffu;
        if (buf.size() + 2 + len > SBE_CE_FALLBACK_REC_MAX) throw std::runtime_error("buffer too short [E100]");
        put16((uint32_t)len);
        buf.insert(buf.end(), v.begin(), v.begin() + len);
    };
    put16(SBE_TM_BLOCK_LEN);
    put16(SBE_TM_TEMPLATE_ID);
    put16(SBE_TOPIC_SCHEMA_ID);
    put16(1);
    put64(now());  // timestamp
    put64(0);      // sequenceNumber
    put_var("_subscriptions");
    put_var("COMMIT_OFFSET");
    put_var(std::string("commit_offset_") + client_id + "_" + std::to_string(now()));
    put_var(text);
    put_var("{}");
    return buf;
}

void CommitManager::commit_message(const std::string& topic, const std::string& message_identifier,
                                   const std::string& message_id, std::uint64_t timestamp_nanos,
                                   std::uint64_t sequence_number) {
    std::lock_guard<std::mutex> lock(commits_mutex_);
    commits_[topic + ":" + message_identifier] =
        CommitOffset{topic, message_identifier, message_id, timestamp_nanos, sequence_number};
}

std::shared_ptr<CommitOffset> CommitManager::get_last_commit(const std::string& topic,
                                                             const std::string& message_identifier) const {
    std::lock_guard<std::mutex> lock(commits_mutex_);
    auto it = commits_.find(topic + ":" + message_identifier);
    return it == commits_.end() ? nullptr : std::make_shared<CommitOffset>(it->second);
}

std::unordered_map<std::string, CommitOffset> CommitManager::get_all_commits() const {
    std::lock_guard<std::mutex> lock(commits_mutex_);
    return commits_;
}

namespace {
// Value::asString of a topic token the device located (jsoncpp 1.9.5).  These four helpers are
// new with AutoCommitter: the mirror had no decode-side JSON code (its Order JSON is written on the
// device).  They convert only tokens that the device reader has already parsed and validated, so
// the string decode cannot fail here and they do not check again.
void utf8_append(uint32_t cp, std::string& out) {
    if (cp <= 0x7f) {
        out += (char)cp;
    } else if (cp <= 0x7ff) {
        out += (char)(0xC0 | (cp >> 6));
        out += (char)(0x80 | (cp & 0x3f));
    } else if (cp <= 0xffff) {
        out += (char)(0xE0 | (cp >> 12));
        out += (char)(0x80 | ((cp >> 6) & 0x3f));
        out += (char)(0x80 | (cp & 0x3f));
    } else if (cp <= 0x10ffff) {
        out += (char)(0xF0 | (cp >> 18));
        out += (char)(0x80 | ((cp >> 12) & 0x3f));
        out += (char)(0x80 | ((cp >> 6) & 0x3f));
        out += (char)(0x80 | (cp & 0x3f));
    }
}
// four hex digits at t[i..i+4): the device's jhex4 accepted them, so a non-hex character or a short
// tail cannot occur and is not diagnosed (a non-hex character would be read as 'A'-based)
uint32_t hex4(std::string_view t, size_t i) {
    uint32_t v = 0;
    for (size_t j = i; j < i + 4 && j < t.size(); ++j) {
        const char c = t[j];
        v = v * 16 + (c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c - 'A' + 10);
    }
    return v;
}
std::string json_unescape(std::string_view t) {  // OurReader::decodeString between the quotes
    std::string out;
    for (size_t i = 0; i < t.size();) {
        const char c = t[i++];
        if (c != '\\' || i == t.size()) {
            out += c;
            continue;
        }
        const char x = t[i++];
        switch (x) {
            case 'b': out += '\b'; break;
            case 'f': out += '\f'; break;
            case 'n': out += '\n'; break;
            case 'r': out += '\r'; break;
            case 't': out += '\t'; break;
            case 'u': {
                uint32_t cp = hex4(t, i);
                i += 4;
                if (cp >= 0xD800 && cp <= 0xDBFF) {  // a surrogate pair: "\uXXXX" follows
                    cp = 0x10000 + ((cp & 0x3FF) << 10) + (hex4(t, i + 2) & 0x3FF);
                    i += 6;
                }
                utf8_append(cp, out);
                break;
            }
            default: out += x; break;  // '"', '/', '\\'
        }
    }
    return out;
}
std::string json_number_as_string(std::string_view t) {  // decodeNumber, then valueToString
    size_t p = 0;
    const bool neg = !t.empty() && t[0] == '-';
    if (neg) ++p;
    const uint64_t maxv = neg ? (uint64_t)1 << 63 : ~0ull, thr = maxv / 10;
    uint64_t v = 0;
    bool real = false;
    while (p < t.size() && !real) {
        const char c = t[p++];
        if (c < '0' || c > '9') {
            real = true;
        } else {
            const uint64_t dg = c - '0';
            if (v >= thr && (v > thr || p != t.size() || dg > maxv % 10)) real = true;
            else v = v * 10 + dg;
        }
    }
    if (!real) return neg ? (v ? "-" + std::to_string(v) : "0") : std::to_string(v);
    const double d = std::strtod(std::string(t).c_str(), nullptr);
    if (d != d) return "null";
    if (d > DBL_MAX) return "1e+9999";
    if (d < -DBL_MAX) return "-1e+9999";
    char buf[40];
    std::snprintf(buf, sizeof buf, "%.17g", d);
    std::string s(buf);
    if (s.find('.') == std::string::npos && s.find('e') == std::string::npos) s += ".0";
    return s;
}
}  // namespace

AutoCommitter::AutoCommitter(std::string client_id, std::string fallback_topic)
    : client_id_(std::move(client_id)), fallback_(std::move(fallback_topic)) {
    if (fallback_.size() > SBE_COMMIT_TABLE_BYTES) throw std::length_error("AutoCommitter: fallback topic too long");
}

void AutoCommitter::set_message_identifier(const std::string& topic, const std::string& identifier) {
    if (!identifiers_.count(topic)) {
        size_t bytes = fallback_.size() + topic.size();
        for (const auto& kv : identifiers_) bytes += kv.first.size();
        if (identifiers_.size() + 2 > SBE_COMMIT_MAX_TOPICS || bytes > SBE_COMMIT_TABLE_BYTES)
            throw std::length_error("AutoCommitter: the topic table holds 64 topics and 4096 bytes");
    }
    identifiers_[topic] = identifier;
}

const std::string& AutoCommitter::message_identifier(const std::string& topic) const {
    auto it = identifiers_.find(topic);
    return it == identifiers_.end() ? client_id_ : it->second;
}

// What commit_and_send_batch asks of run() beyond the plan, and what it gets back.
struct AutoCommitter::EmitRequest {
    const CommitSendOptions* options;
    const std::vector<bool>* callback_ok;
    std::vector<std::uint8_t> status;    // [n] SBE_CE_*
    std::vector<std::uint64_t> out_off;  // [n + 1]
    std::vector<std::uint8_t> frames;    // out_off[n] bytes
    std::uint64_t now_ns = 0, uuid_ns = 0;  // json_fallback: the call's two clock readings
};

CommitPlan AutoCommitter::classify(const ParsedBatch& batch) const { return run(batch, nullptr); }

CommitPlan AutoCommitter::run(const ParsedBatch& batch, EmitRequest* emit) const {
    const size_t n = batch.n_;
    CommitPlan plan;
    plan.table.push_back(fallback_);
    for (const auto& kv : identifiers_) plan.table.push_back(kv.first);
    const uint32_t k = (uint32_t)plan.table.size();
    plan.cm.resize(n);
    plan.topic_src.resize(n);
    plan.topic_kind.resize(n);
    plan.topic_off.resize(n);
    plan.topic_len.resize(n);
    plan.topic_idx.resize(n);
    plan.last.assign(k, ~0ull);
    plan.count.assign(k + 2, 0);
    if (emit) {
        emit->status.assign(n, SBE_CE_NONE);
        emit->out_off.assign(n + 1, 0);
        emit->frames.clear();
    }
    if (n == 0) return plan;
    const Descriptors& d = *batch.desc_;
    const uint64_t lo = batch.rec_off_[0], bytes = batch.rec_off_[n] - lo;
    const bool fallback = emit && emit->options->json_fallback;
    if (fallback && client_id_.size() > SBE_COMMIT_TABLE_BYTES)
        throw std::length_error("AutoCommitter: the default identifier holds 4096 bytes");
    // staged inputs: offsets (rebased), status, flags, view offsets and lengths, the table, the records
    const size_t o_st = al16((n + 1) * 8), o_fl = o_st + al16(n), o_vo = o_fl + al16(n), o_vl = o_vo + al16(20 * n),
                 o_ta = o_vl + al16(20 * n), o_to = o_ta + SBE_COMMIT_TABLE_BYTES,
                 o_tid = o_to + al16(4 * (SBE_COMMIT_MAX_TOPICS + 1)),
                 // emit only: topic ids, the identifier table, sequence numbers, the callback mask
                 o_ia = o_tid + (emit ? al16(4 * SBE_COMMIT_MAX_TOPICS) : 0),
                 o_io = o_ia + (emit ? SBE_COMMIT_TABLE_BYTES : 0),
                 o_seq = o_io + (emit ? al16(4 * (SBE_COMMIT_MAX_TOPICS + 1)) : 0), o_mask = o_seq + (emit ? al16(8 * n) : 0),
                 // json_fallback only: the records' timestamps, the default identifier (client_id)
                 o_ts = o_mask + (emit ? al16(n) : 0), o_di = o_ts + (fallback ? al16(8 * n) : 0),
                 o_data = o_di + (fallback ? SBE_COMMIT_TABLE_BYTES : 0), stage = o_data + (size_t)bytes + 16;
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // serial use of the pipeline's first slot (idle between calls)
    hipStream_t stream = c.batch_stream();
    s.pin.need(stage);
    uint8_t* hp = s.pin.b();
    uint64_t* ro = reinterpret_cast<uint64_t*>(hp);
    uint32_t* vo = reinterpret_cast<uint32_t*>(hp + o_vo);
    uint32_t* vl = reinterpret_cast<uint32_t*>(hp + o_vl);
    ro[n] = bytes;
    for_ranges(n, 4096, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) {
            ro[i] = batch.rec_off_[i] - lo;
            hp[o_st + i] = d.status(i);
            hp[o_fl + i] = d.flags(i);
            std::memcpy(vo + 5 * i, d.off(i), 20);
            std::memcpy(vl + 5 * i, d.len(i), 20);
        }
    });
    std::memset(hp + o_ta, 0, SBE_COMMIT_TABLE_BYTES);
    uint32_t* to = reinterpret_cast<uint32_t*>(hp + o_to);
    to[0] = 0;
    for (uint32_t j = 0; j < k; ++j) {
        std::memcpy(hp + o_ta + to[j], plan.table[j].data(), plan.table[j].size());
        to[j + 1] = to[j] + (uint32_t)plan.table[j].size();
    }
    const bool masked = emit && emit->callback_ok;
    size_t ident_max = 0;
    if (emit) {  // topic_to_id and message_identifier of every table entry
        uint32_t* tid = reinterpret_cast<uint32_t*>(hp + o_tid);
        uint32_t* io = reinterpret_cast<uint32_t*>(hp + o_io);
        std::memset(hp + o_ia, 0, SBE_COMMIT_TABLE_BYTES);
        io[0] = 0;
        for (uint32_t j = 0; j < k; ++j) {
            const std::string& id = message_identifier(plan.table[j]);
            if (io[j] + id.size() > SBE_COMMIT_TABLE_BYTES)
                throw std::length_error("AutoCommitter: the identifier table holds 4096 bytes");
            tid[j] = CommitManager::topic_to_id(plan.table[j]);
            std::memcpy(hp + o_ia + io[j], id.data(), id.size());
            io[j + 1] = io[j] + (uint32_t)id.size();
            ident_max = std::max(ident_max, id.size());
        }
        uint64_t* sq = reinterpret_cast<uint64_t*>(hp + o_seq);
        for_ranges(n, 4096, [&](size_t x, size_t y) {
            for (size_t i = x; i < y; ++i) {
                sq[i] = d.seq(i);
                if (masked) hp[o_mask + i] = (*emit->callback_ok)[i] ? 1 : 0;
                if (fallback) reinterpret_cast<uint64_t*>(hp + o_ts)[i] = (uint64_t)batch.timestamp(i);
            }
        });
        if (fallback) {
            std::memcpy(hp + o_di, client_id_.data(), client_id_.size());
            ident_max = std::max(ident_max, client_id_.size());
        }
    }
    if (bytes)
        for_ranges((size_t)bytes, size_t(1) << 18, [&](size_t x, size_t y) {
            std::memcpy(hp + o_data + x, batch.data_ + lo + x, y - x);
        });
    s.d_in.need(stage);
    const size_t p_src = al16(n), p_kind = p_src + al16(n), p_off = p_kind + al16(n), p_len = p_off + al16(4 * n),
                 p_idx = p_len + al16(4 * n), p_last = p_idx + al16(4 * n), p_cnt = p_last + 8 * SBE_COMMIT_MAX_TOPICS,
                 outb = p_cnt + 8 * (SBE_COMMIT_MAX_TOPICS + 2);
    // emit only: status, offsets, totals, the workspace and the frames
    const int framed = emit && emit->options->session_frame ? 1 : 0;
    const size_t wsb = emit ? sbe_commit_emit_workspace_size(n) : 0,
                 bound = !emit      ? 0
                         : fallback ? (size_t)sbe_commit_fallback_output_bound(n, bytes + n * ident_max, framed)
                                    : (size_t)sbe_commit_emit_output_bound(n, bytes + n * ident_max, framed),
                 p_est = outb, p_eoff = p_est + al16(n), p_tot = p_eoff + al16(8 * (n + 1)), p_ws = p_tot + 32,
                 p_frames = p_ws + al16(wsb);
    s.d_out.need(emit ? p_frames + bound : outb);
    hip_check(hipMemcpyAsync(s.d_in.p, hp, stage, hipMemcpyHostToDevice, stream), "H2D");
    uint8_t* di = s.d_in.b();
    uint8_t* dq = s.d_out.b();
    sbe_decoded dec{di + o_st, di + o_fl, nullptr, nullptr, reinterpret_cast<uint32_t*>(di + o_vo),
                    reinterpret_cast<uint32_t*>(di + o_vl), nullptr};
    sbe_commit_out out{dq,
                       dq + p_src,
                       dq + p_kind,
                       reinterpret_cast<uint32_t*>(dq + p_off),
                       reinterpret_cast<uint32_t*>(dq + p_len),
                       reinterpret_cast<uint32_t*>(dq + p_idx),
                       reinterpret_cast<uint64_t*>(dq + p_last),
                       reinterpret_cast<uint64_t*>(dq + p_cnt)};
    if (sbe_classify_commits(di + o_data, reinterpret_cast<const uint64_t*>(di), n, &dec, di + o_ta,
                             reinterpret_cast<const uint32_t*>(di + o_to), k, &out, nullptr, 0, stream) != SBE_OK) {
        c.abort_all();
        fail("sbe_classify_commits");
    }
    if (emit) {  // the plan is read where classify wrote it
        const sbe_decoded dec_seq{dec.status,   dec.flags,    nullptr, fallback ? reinterpret_cast<uint64_t*>(di + o_ts) : nullptr,
                                  dec.view_off, dec.view_len, reinterpret_cast<uint64_t*>(di + o_seq)};
        const sbe_commit_fallback fb{di + o_ta,      reinterpret_cast<const uint32_t*>(di + o_to),
                                     di + o_di,      (uint32_t)client_id_.size(),
                                     emit->now_ns,   emit->uuid_ns};
        const sbe_commit_emit_out res{reinterpret_cast<uint64_t*>(dq + p_eoff), dq + p_est, nullptr,
                                      reinterpret_cast<uint64_t*>(dq + p_tot)};
        if (sbe_emit_commit_offsets_ex(di + o_data, reinterpret_cast<const uint64_t*>(di), n, &dec_seq, &out,
                                       reinterpret_cast<const uint32_t*>(di + o_tid), di + o_ia,
                                       reinterpret_cast<const uint32_t*>(di + o_io), k, masked ? di + o_mask : nullptr,
                                       emit->options->last_only ? SBE_CE_LAST_ONLY : 0u, framed,
                                       emit->options->leadership_term_id, emit->options->cluster_session_id,
                                       dq + p_frames, bound, &res, dq + p_ws, wsb, stream,
                                       fallback ? &fb : nullptr) != SBE_OK) {
            c.abort_all();
            fail("sbe_emit_commit_offsets");
        }
    }
    auto back = [&](void* dst, size_t off, size_t len) {
        hip_check(hipMemcpyAsync(dst, dq + off, len, hipMemcpyDeviceToHost, stream), "D2H");
    };
    back(plan.cm.data(), 0, n);
    back(plan.topic_src.data(), p_src, n);
    back(plan.topic_kind.data(), p_kind, n);
    back(plan.topic_off.data(), p_off, 4 * n);
    back(plan.topic_len.data(), p_len, 4 * n);
    back(plan.topic_idx.data(), p_idx, 4 * n);
    back(plan.last.data(), p_last, 8 * k);
    back(plan.count.data(), p_cnt, 8 * (k + 2));
    if (emit) {
        back(emit->status.data(), p_est, n);
        back(emit->out_off.data(), p_eoff, 8 * (n + 1));
    }
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    if (emit && emit->out_off[n]) {  // the bound holds every frame: none overflowed
        emit->frames.resize((size_t)emit->out_off[n]);
        back(emit->frames.data(), p_frames, emit->frames.size());
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    }
    return plan;
}

std::string AutoCommitter::topic(const ParsedBatch& batch, const CommitPlan& plan, std::size_t i) const {
    if (plan.topic_src[i] == SBE_TOPIC_SRC_FALLBACK || plan.topic_src[i] == SBE_TOPIC_SRC_NONE) return fallback_;
    const std::string_view tok(reinterpret_cast<const char*>(batch.data_ + batch.rec_off_[i]) + plan.topic_off[i],
                               plan.topic_len[i]);
    switch (plan.topic_kind[i]) {
        case SBE_TOPIC_KIND_STRING: return std::string(tok);
        case SBE_TOPIC_KIND_STRING_ESC: return json_unescape(tok);
        case SBE_TOPIC_KIND_NUMBER: return json_number_as_string(tok);
        case SBE_TOPIC_KIND_TRUE: return "true";
        case SBE_TOPIC_KIND_FALSE: return "false";
        default: return "";  // null
    }
}

std::size_t AutoCommitter::commit_record_by_record(const ParsedBatch& batch, const CommitPlan& plan,
                                                   CommitManager& commits, const std::vector<bool>* callback_ok) const {
    std::size_t calls = 0;
    for (std::size_t i = 0; i < batch.size(); ++i) {
        if (plan.cm[i] != SBE_CM_COMMIT || (callback_ok && !(*callback_ok)[i])) continue;
        const std::string t = topic(batch, plan, i);
        commits.commit_message(t, message_identifier(t), std::string(batch.view(i, 2)),
                               (std::uint64_t)batch.timestamp(i), batch.sequence_number(i));
        ++calls;
    }
    return calls;
}

std::size_t AutoCommitter::commit_batch(const ParsedBatch& batch, const CommitPlan& plan, CommitManager& commits,
                                        const std::vector<bool>* callback_ok) const {
    if (callback_ok) {
        if (callback_ok->size() != batch.size()) throw std::invalid_argument("AutoCommitter: one callback result per record");
        return commit_record_by_record(batch, plan, commits, callback_ok);
    }
    // the last committable record of every table entry, and every record the table does not
    // resolve, in record order (two topics can spell one "topic:identifier" key)
    std::vector<std::size_t> todo;
    for (std::size_t j = 0; j < plan.last.size(); ++j)
        if (plan.last[j] != ~0ull) todo.push_back((std::size_t)plan.last[j]);
    if (plan.count[plan.last.size()] + plan.count[plan.last.size() + 1])
        for (std::size_t i = 0; i < batch.size(); ++i)
            if (plan.cm[i] == SBE_CM_COMMIT && plan.topic_idx[i] >= SBE_TOPIC_HOST) todo.push_back(i);
    std::sort(todo.begin(), todo.end());
    for (std::size_t i : todo) {
        const std::string t = plan.topic_idx[i] < plan.table.size() ? plan.table[plan.topic_idx[i]] : topic(batch, plan, i);
        commits.commit_message(t, message_identifier(t), std::string(batch.view(i, 2)),
                               (std::uint64_t)batch.timestamp(i), batch.sequence_number(i));
    }
    return todo.size();
}

std::size_t AutoCommitter::commit_batch(const ParsedBatch& batch, CommitManager& commits,
                                        const std::vector<bool>* callback_ok) const {
    return commit_batch(batch, classify(batch), commits, callback_ok);
}

CommitSendResult AutoCommitter::commit_and_send_batch(const ParsedBatch& batch, CommitManager& commits,
                                                      const OfferFn& offer, const CommitSendOptions& options,
                                                      const std::vector<bool>* callback_ok) const {
    if (callback_ok && callback_ok->size() != batch.size())
        throw std::invalid_argument("AutoCommitter: one callback result per record");
    if (callback_ok && options.last_only)
        throw std::invalid_argument("AutoCommitter: last_only sends what an unmasked commit_batch commits");
    EmitRequest emit{&options, callback_ok, {}, {}, {}, 0, 0};
    if (options.json_fallback) {  // the call's two clock readings: timestamp, then uuid
        emit.now_ns = options.clock ? options.clock() : now_nanos_sys();
        emit.uuid_ns = options.clock ? options.clock() : now_nanos_sys();
    }
    const CommitPlan plan = run(batch, &emit);
    CommitSendResult r;
    r.commits = commit_batch(batch, plan, commits, callback_ok);
    std::vector<std::uint8_t> frame;
    auto send = [&](const std::uint8_t* p, std::size_t len) {
        ++r.offered;
        if (offer(p, len)) ++r.accepted;
    };
    auto session_header = [&] {  // `frame` = the SessionMessageHeader (src/session_manager.cpp:936-967), or empty
        frame.clear();
        if (!options.session_frame) return;
        const std::uint16_t h[4] = {SBE_SESSION_BLOCK_LEN, SBE_SESSION_TEMPLATE_ID, SBE_CLUSTER_SCHEMA_ID,
                                    SBE_CLUSTER_SCHEMA_VERSION};
        const std::int64_t ids[3] = {options.leadership_term_id, options.cluster_session_id, 0};
        frame.resize(SBE_SESSION_HDR_LEN);
        std::memcpy(frame.data(), h, 8);  // little-endian host, as the rest of the mirror
        std::memcpy(frame.data() + 8, ids, 24);
    };
    for (std::size_t i = 0; i < batch.size(); ++i) {
        const std::uint8_t st = emit.status[i];
        if (st == SBE_CE_EMITTED || st == SBE_CE_EMITTED_JSON) {
            send(emit.frames.data() + emit.out_off[i], (std::size_t)(emit.out_off[i + 1] - emit.out_off[i]));
        } else if (st == SBE_CE_E109_MESSAGE_ID) {
            r.too_long.push_back(i);
        } else if (st == SBE_CE_E100_FALLBACK) {
            r.fallback_e100.push_back(i);
        } else if (st == SBE_CE_HOST) {
            const bool entry = plan.topic_idx[i] < plan.table.size();  // a table entry whose topic has id 0
            if (options.last_only && entry && plan.last[plan.topic_idx[i]] != i) continue;
            const std::string t = entry ? plan.table[plan.topic_idx[i]] : topic(batch, plan, i);
            const std::string_view id = batch.view(i, 2);
            if (CommitManager::topic_to_id(t) == 0) {
                if (!options.json_fallback) {
                    r.unsent.push_back(i);
                    continue;
                }
                // the device's convention: the call's first reading, then the second + i
                const CommitOffset off{t, message_identifier(t), std::string(id), (std::uint64_t)batch.timestamp(i),
                                       batch.sequence_number(i)};
                int reads = 0;
                try {
                    const std::vector<std::uint8_t> rec = commits.build_commit_offset_fallback(
                        off.message_identifier, off, [&] { return reads++ ? emit.uuid_ns + i : emit.now_ns; });
                    session_header();
                    frame.insert(frame.end(), rec.begin(), rec.end());
                    send(frame.data(), frame.size());
                } catch (const std::runtime_error&) {  // "buffer too short [E100]"
                    r.fallback_e100.push_back(i);
                }
                continue;
            }
            if (id.size() > SBE_VAR_MAX_LEN) {
                r.too_long.push_back(i);
                continue;
            }
            const CommitOffset off{t, message_identifier(t), std::string(id), (std::uint64_t)batch.timestamp(i),
                                   batch.sequence_number(i)};
            const std::vector<std::uint8_t> rec = commits.build_commit_offset_message(t, client_id_, off);
            session_header();
            frame.insert(frame.end(), rec.begin(), rec.end());
            send(frame.data(), frame.size());
        }
    }
    return r;
}

OrderJsonBatch orders_to_json(const std::vector<Order>& orders, const std::vector<std::string>& message_ids) {
    const size_t n = orders.size();
    if (message_ids.size() != n) throw std::invalid_argument("orders_to_json: one message id per order");
    OrderJsonBatch r;
    for (EncodedBatch* b : {&r.payload, &r.headers}) {
        b->offsets = HostBytesAccess::make<uint64_t>(n + 1);
        b->status = HostBytesAccess::make<uint8_t>(n);
        HostBytesAccess::zero(b->offsets);
        HostBytesAccess::zero(b->status);
    }
    if (n == 0) return r;
    auto field = [&](size_t i, int k) -> std::string_view {
        const Order& o = orders[i];
        switch (k) {
            case 0: return o.client_order_uuid;
            case 1: return o.identifier;
            case 2: return o.base_token;
            case 3: return o.quote_token;
            case 4: return o.side;
            case 5: return o.id;
            case 6: return message_ids[i];
            default: return o.status;
        }
    };
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // serial use of the pipeline's first slot (idle between calls)
    hipStream_t stream = c.batch_stream();
    std::vector<uint64_t> pin;
    prefix(n, pin, [&](size_t i) {
        uint64_t t = 0;
        for (int k = 0; k < (int)SBE_ORDER_FIELDS; ++k) t += field(i, k).size();
        return t;
    });
    const size_t arena = (size_t)pin[n];
    const size_t o_len = al16(arena), nlen = n * 4 * SBE_ORDER_FIELDS, o_num = o_len + al16(nlen), stage = o_num + n * 24;
    s.pin.need(stage);
    uint8_t* ap = s.pin.b();
    uint32_t* lp = reinterpret_cast<uint32_t*>(ap + o_len);
    int64_t* cid = reinterpret_cast<int64_t*>(ap + o_num);
    int64_t* ts = cid + n;
    double* q = reinterpret_cast<double*>(ts + n);
    for_ranges(n, 2048, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) {
            uint8_t* at = ap + pin[i];
            for (int k = 0; k < (int)SBE_ORDER_FIELDS; ++k) {
                const std::string_view f = field(i, k);
                if (!f.empty()) std::memcpy(at, f.data(), f.size());
                at += f.size();
                lp[SBE_ORDER_FIELDS * i + k] = (uint32_t)f.size();
            }
            cid[i] = orders[i].customer_id;
            ts[i] = orders[i].timestamp;
            q[i] = orders[i].quantity;
        }
    });
    // a record is at most ~800 B besides its strings (428 fixed, 316 for "%f" of a quantity near
    // DBL_MAX, 24 for "%.17g", 34 for two integers); strings escape to <= 6x and appear <= twice.
    // out_off always holds the full sizes, so a record past the capacity is redone below.
    uint64_t cap = 12 * (uint64_t)arena + 900 * (uint64_t)n + 16;
    s.d_in.need(stage);
    const size_t o_off = 0, o_st = al16(2 * (n + 1) * 8), o_ws = o_st + al16(2 * n);
    const size_t wsb = sbe_order_json_workspace_size(n);
    c.d_aux.need(o_ws + wsb);
    hip_check(hipMemcpyAsync(s.d_in.p, ap, stage, hipMemcpyHostToDevice, stream), "H2D");
    const uint8_t* di = s.d_in.b();
    const int64_t* d_cid = reinterpret_cast<const int64_t*>(di + o_num);
    sbe_order_batch in{di, nullptr, reinterpret_cast<const uint32_t*>(di + o_len), d_cid, d_cid + n,
                       reinterpret_cast<const double*>(d_cid + 2 * n)};
    for (int w = 0; w < 2; ++w) {
        EncodedBatch& b = w ? r.headers : r.payload;
        uint64_t* off = reinterpret_cast<uint64_t*>(c.d_aux.b() + o_off) + w * (n + 1);
        uint8_t* st = c.d_aux.b() + o_st + w * n;
        for (int attempt = 0;; ++attempt) {
            s.d_out.need(cap);
            if (sbe_order_to_json_batch(&in, n, w ? SBE_JSON_PUBLISH_HEADERS : SBE_JSON_ORDER_PAYLOAD, s.d_out.b(), cap,
                                        off, st, c.d_aux.b() + o_ws, wsb, stream) != SBE_OK)
                fail("sbe_order_to_json_batch");
            hip_check(hipMemcpyAsync(b.offsets.data(), off, (n + 1) * 8, hipMemcpyDeviceToHost, stream), "D2H");
            hip_check(hipMemcpyAsync(b.status.data(), st, n, hipMemcpyDeviceToHost, stream), "D2H");
            hip_check(hipStreamSynchronize(stream), "sync");
            if (b.offsets[n] <= cap || attempt > 0) break;
            cap = b.offsets[n];  // the measured size: one rerun
        }
        for (size_t i = 0; i < n; ++i)
            if (b.status[i] != SBE_JSON_OK) throw std::runtime_error("sbecodec: order JSON record did not fit");
        b.bytes = HostBytesAccess::make((size_t)b.offsets[n]);
        if (b.offsets[n]) {
            hip_check(hipMemcpyAsync(b.bytes.data(), s.d_out.p, b.offsets[n], hipMemcpyDeviceToHost, stream), "D2H");
            hip_check(hipStreamSynchronize(stream), "sync");
        }
    }
    return r;
}

std::string Order::to_json() const {
    OrderJsonBatch b = orders_to_json({*this}, {std::string()});
    return std::string(b.payload.bytes.begin(), b.payload.bytes.end());
}

// ---- Order::validate and the fused publish path ----
namespace {
const char* const kValidateText[SBE_PUB_INVALID_COUNT] = {
    "Order ID is required",
    "Base token is required",
    "Quote token is required",
    "Side must be 'BUY' or 'SELL'",
    "Quantity must be positive",
    "Invalid order type: ",
    "Limit price must be positive for LIMIT orders",
    "Stop price must be positive for STOP orders",
    "Stop price must be positive for STOP_LIMIT orders",
    "Limit price must be positive for STOP_LIMIT orders",
    "Invalid time in force: ",
    "Expiry timestamp required for GTD orders"};

std::string default_message_id() {  // src/order_types.cpp:428-437
    const int64_t ts = std::chrono::high_resolution_clock::now().time_since_epoch().count();
    thread_local std::mt19937 gen{std::random_device{}()};
    std::uniform_int_distribution<uint32_t> dis(10000, 99999);
    return "msg_" + std::to_string(ts) + "_" + std::to_string(dis(gen));
}
}  // namespace

std::vector<std::string> Order::validate() const {
    std::vector<std::string> errors;
    if (id.empty()) errors.push_back("Order ID is required");
    if (base_token.empty()) errors.push_back("Base token is required");
    if (quote_token.empty()) errors.push_back("Quote token is required");
    if (!(side == "BUY" || side == "SELL")) errors.push_back("Side must be 'BUY' or 'SELL'");
    if (quantity <= 0.0) errors.push_back("Quantity must be positive");
    if (!(order_type == "MARKET" || order_type == "LIMIT" || order_type == "STOP" || order_type == "STOP_LIMIT"))
        errors.push_back("Invalid order type: " + order_type);
    if (order_type == "LIMIT" && limit_price <= 0.0) errors.push_back("Limit price must be positive for LIMIT orders");
    if (order_type == "STOP" && (!stop_price.has_value() || stop_price.value() <= 0.0))
        errors.push_back("Stop price must be positive for STOP orders");
    if (order_type == "STOP_LIMIT") {
        if (!stop_price.has_value() || stop_price.value() <= 0.0)
            errors.push_back("Stop price must be positive for STOP_LIMIT orders");
        if (limit_price <= 0.0) errors.push_back("Limit price must be positive for STOP_LIMIT orders");
    }
    if (!(time_in_force == "GTC" || time_in_force == "IOC" || time_in_force == "FOK" || time_in_force == "DAY" ||
          time_in_force == "GTD"))
        errors.push_back("Invalid time in force: " + time_in_force);
    if (time_in_force == "GTD" && !expiry_timestamp.has_value())
        errors.push_back("Expiry timestamp required for GTD orders");
    return errors;
}

OrderPublisher::OrderPublisher(OfferFn offer, std::string default_topic, OrderPublisherOptions options)
    : offer_(std::move(offer)), default_topic_(std::move(default_topic)), opt_(std::move(options)) {
    if (!opt_.message_id) opt_.message_id = default_message_id;
    if (!opt_.clock)
        opt_.clock = [] { return (uint64_t)std::chrono::high_resolution_clock::now().time_since_epoch().count(); };
}

std::string OrderPublisher::validation_message(unsigned k, const Order& order) {
    if (k >= SBE_PUB_INVALID_COUNT) return std::string();
    std::string m = kValidateText[k];
    if (k == SBE_PUB_INVALID_ORDER_TYPE - SBE_PUB_INVALID_ID) m += order.order_type;
    if (k == SBE_PUB_INVALID_TIME_IN_FORCE - SBE_PUB_INVALID_ID) m += order.time_in_force;
    return m;
}

PublishedOrders OrderPublisher::publish_orders_batch(const std::vector<Order>& orders) {
    return publish_orders_batch_to_topic(orders, default_topic_);
}

PublishedOrders OrderPublisher::publish_orders_batch_to_topic(const std::vector<Order>& orders,
                                                              const std::string& topic) {
    const size_t n = orders.size();
    PublishedOrders r;
    r.message_ids.resize(n);
    r.status.assign(n, 0);
    r.error_mask.assign(n, 0);
    if (n == 0) return r;
    std::vector<uint64_t> tm_ts(n);
    for (size_t i = 0; i < n; ++i) {  // in order: injected generators may count
        r.message_ids[i] = opt_.message_id();
        tm_ts[i] = opt_.clock();
    }
    auto field = [&](size_t i, int k) -> std::string_view {
        const Order& o = orders[i];
        switch (k) {
            case 0: return o.client_order_uuid;
            case 1: return o.identifier;
            case 2: return o.base_token;
            case 3: return o.quote_token;
            case 4: return o.side;
            case 5: return o.id;
            case 6: return r.message_ids[i];
            default: return o.status;
        }
    };
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // serial use of the pipeline's first slot (idle between calls)
    hipStream_t stream = c.batch_stream();
    std::vector<uint64_t> pin, cpin;
    prefix(n, pin, [&](size_t i) {
        uint64_t t = 0;
        for (int k = 0; k < (int)SBE_ORDER_FIELDS; ++k) t += field(i, k).size();
        return t;
    });
    prefix(n, cpin, [&](size_t i) { return (uint64_t)(orders[i].order_type.size() + orders[i].time_in_force.size()); });
    // staging layout: order arena | order lengths | customer_id, timestamp, quantity, limit, stop,
    // TopicMessage timestamps (8 B each) | checks lengths | present | checks arena | topic
    const size_t arena = (size_t)pin[n], carena = (size_t)cpin[n];
    const size_t o_len = al16(arena), o_num = o_len + al16(n * 4 * SBE_ORDER_FIELDS), o_clen = o_num + n * 48,
                 o_pres = o_clen + al16(n * 8), o_car = o_pres + al16(n), o_topic = o_car + al16(carena),
                 stage = o_topic + al16(topic.size());
    s.pin.need(stage);
    uint8_t* ap = s.pin.b();
    uint32_t* lp = reinterpret_cast<uint32_t*>(ap + o_len);
    int64_t* cid = reinterpret_cast<int64_t*>(ap + o_num);
    int64_t* ts = cid + n;
    double* q = reinterpret_cast<double*>(ts + n);
    double* lim = q + n;
    double* stop = lim + n;
    uint64_t* tts = reinterpret_cast<uint64_t*>(stop + n);
    uint32_t* clp = reinterpret_cast<uint32_t*>(ap + o_clen);
    uint8_t* pres = ap + o_pres;
    for_ranges(n, 2048, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) {
            const Order& o = orders[i];
            uint8_t* at = ap + pin[i];
            for (int k = 0; k < (int)SBE_ORDER_FIELDS; ++k) {
                const std::string_view f = field(i, k);
                if (!f.empty()) std::memcpy(at, f.data(), f.size());
                at += f.size();
                lp[SBE_ORDER_FIELDS * i + k] = (uint32_t)f.size();
            }
            cid[i] = o.customer_id;
            ts[i] = o.timestamp;
            q[i] = o.quantity;
            lim[i] = o.limit_price;
            stop[i] = o.stop_price.value_or(0.0);
            tts[i] = tm_ts[i];
            pres[i] = (uint8_t)((o.stop_price.has_value() ? SBE_PUB_HAS_STOP_PRICE : 0u) |
                                (o.expiry_timestamp.has_value() ? SBE_PUB_HAS_EXPIRY : 0u));
            uint8_t* cat = ap + o_car + cpin[i];
            if (!o.order_type.empty()) std::memcpy(cat, o.order_type.data(), o.order_type.size());
            if (!o.time_in_force.empty())
                std::memcpy(cat + o.order_type.size(), o.time_in_force.data(), o.time_in_force.size());
            clp[2 * i] = (uint32_t)o.order_type.size();
            clp[2 * i + 1] = (uint32_t)o.time_in_force.size();
        }
    });
    if (!topic.empty()) std::memcpy(ap + o_topic, topic.data(), topic.size());
    s.d_in.need(stage);
    hip_check(hipMemcpyAsync(s.d_in.p, ap, stage, hipMemcpyHostToDevice, stream), "H2D");
    const uint8_t* di = s.d_in.b();
    const int64_t* d_cid = reinterpret_cast<const int64_t*>(di + o_num);
    const double* d_q = reinterpret_cast<const double*>(d_cid + 2 * n);
    sbe_order_batch in{di, nullptr, reinterpret_cast<const uint32_t*>(di + o_len), d_cid, d_cid + n, d_q};
    sbe_order_checks chk{di + o_car, nullptr, reinterpret_cast<const uint32_t*>(di + o_clen), d_q + n, d_q + 2 * n,
                         di + o_pres};
    const uint64_t* d_tts = reinterpret_cast<const uint64_t*>(d_q + 3 * n);
    const size_t o_st = al16((n + 1) * 8), o_mask = o_st + al16(n), o_ws = o_mask + al16(2 * n);
    const size_t wsb = sbe_publish_orders_workspace_size(n);
    c.d_aux.need(o_ws + wsb);
    uint64_t* d_off = reinterpret_cast<uint64_t*>(c.d_aux.b());
    uint8_t* d_st = c.d_aux.b() + o_st;
    uint16_t* d_mask = reinterpret_cast<uint16_t*>(c.d_aux.b() + o_mask);
    std::vector<uint64_t> off(n + 1);
    // a typical framed record is ~760 B; out_off always holds the full layout, so a short guess is
    // redone once at the measured size
    uint64_t cap = (1024 + (uint64_t)topic.size()) * n + 2 * (uint64_t)arena + 64;
    for (int attempt = 0;; ++attempt) {
        s.d_out.need(cap);
        if (sbe_publish_orders_batch(&in, &chk, n, topic.empty() ? nullptr : di + o_topic, (uint32_t)topic.size(), d_tts,
                                     0, opt_.reference_truncate8 ? SBE_ENC_REF_TRUNCATE8 : 0u,
                                     opt_.session_framed ? 1 : 0, opt_.leadership_term_id, opt_.cluster_session_id,
                                     s.d_out.b(), cap, d_off, d_st, d_mask, c.d_aux.b() + o_ws, wsb, stream) != SBE_OK)
            fail("sbe_publish_orders_batch");
        hip_check(hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, stream), "D2H");
        hip_check(hipStreamSynchronize(stream), "sync");
        if (off[n] <= cap || attempt > 0) break;
        cap = off[n];
    }
    hip_check(hipMemcpyAsync(r.status.data(), d_st, n, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipMemcpyAsync(r.error_mask.data(), d_mask, 2 * n, hipMemcpyDeviceToHost, stream), "D2H");
    std::vector<uint8_t> bytes((size_t)off[n]);
    if (off[n]) hip_check(hipMemcpyAsync(bytes.data(), s.d_out.p, off[n], hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    for (size_t i = 0; i < n; ++i) {
        if (r.status[i] != SBE_ENC_OK) continue;
        if (!offer_(bytes.data() + off[i], (size_t)(off[i + 1] - off[i]))) break;
        ++r.offered;
    }
    return r;
}

namespace {
std::string publish_one(OrderPublisher& p, const Order& order, const std::string& topic) {
    // validate() on the host first, as the reference does (src/cluster_client.cpp:303-306): an
    // invalid order makes no message id, reads no clock and costs no device call
    const std::vector<std::string> errors = order.validate();
    if (!errors.empty()) throw InvalidMessageException("Order validation failed: " + errors[0]);
    const PublishedOrders r = p.publish_orders_batch_to_topic({order}, topic);
    const uint8_t st = r.status[0];
    if (st >= SBE_PUB_INVALID_ID && st < SBE_PUB_INVALID_ID + SBE_PUB_INVALID_COUNT)  // the device's verdict is the same
        throw InvalidMessageException("Order validation failed: " +
                                      OrderPublisher::validation_message(st - SBE_PUB_INVALID_ID, order));
    // E109 makes create_topic_message throw, publish_message return false (src/session_manager.cpp:1111-1114);
    // a refused offer does the same: the reference's base message (src/cluster_client.cpp:325-329)
    if (st != SBE_ENC_OK || r.offered != 1) throw ClusterClientException("Failed to publish order message");
    return r.message_ids[0];
}
}  // namespace

std::string OrderPublisher::publish_order(const Order& order) { return publish_one(*this, order, default_topic_); }

std::string OrderPublisher::publish_order_to_topic(const Order& order, const std::string& topic) {
    if (topic.empty()) throw InvalidMessageException("Topic is empty");  // src/cluster_client.cpp:338-340
    return publish_one(*this, order, topic);
}

// ======================================================================================
// decode
// ======================================================================================
ParseResult MessageParser::parse_message(const std::uint8_t* data, std::size_t length) {
    if (!data || length == 0) {  // src/sbe_encoder.cpp:516-519 (no device round trip needed)
        ParseResult r;
        r.error_message = "Null or empty data";
        return r;
    }
    const uint64_t off[2] = {0, length};
    auto d = run_decode(data, off, 1, SBE_DEC_PARSE_MESSAGE);
    return materialize(data, *d, 0);
}

ParseResult MessageParser::decode_topic_message_with_sbe(const std::uint8_t* data, std::size_t length) {
    ParseResult r;
    if (!data || length < SBEConstants::SBE_HEADER_LENGTH) {  // MessageHeader::wrap (MessageHeader.h:165-168)
        r.error_message = "SBE TopicMessage decoding failed: buffer too short for flyweight [E107]";
        return r;
    }
    const uint16_t tmpl = rdu16(data + 2), schema = rdu16(data + 4);
    if (tmpl != SBEConstants::TOPIC_MESSAGE_TEMPLATE_ID || schema != SBEConstants::TOPIC_SCHEMA_ID) {  // :976-983
        r.error_message = "Not a TopicMessage (got template_id=" + std::to_string(tmpl) +
                          ", schema_id=" + std::to_string(schema) + ")";
        return r;
    }
    // template 1 / schema 1: parse_message dispatches straight to this function (:539-541, :812-816)
    return parse_message(data, length);
}

ParseResult MessageParser::decode_acknowledgment_with_sbe(const std::uint8_t* data, std::size_t length) {
    ParseResult r;
    if (!data || length < SBEConstants::SBE_HEADER_LENGTH) {  // :842-845
        r.error_message = "Buffer too short for SBE header";
        return r;
    }
    const uint16_t tmpl = rdu16(data + 2), schema = rdu16(data + 4);
    if (tmpl != SBEConstants::ACKNOWLEDGMENT_TEMPLATE_ID || schema != SBEConstants::TOPIC_SCHEMA_ID) {  // :859-865
        r.error_message = "Message is not an Acknowledgment. Expected: template_id=2, schema_id=1. Got: template_id=" +
                          std::to_string(tmpl) + ", schema_id=" + std::to_string(schema);
        return r;
    }
    // template 2 / schema 1: is_topic_message()'s third clause sends parse_message here (:539-541, :817-819)
    return parse_message(data, length);
}

ParseResult MessageParser::parse_message_debug(const std::uint8_t* data, std::size_t length, const std::string& debug_prefix) {
    debug_log(debug_prefix, "📋 Parsing message (", length, " bytes)");
    if (length > 0 && length <= 200) {
        debug_log(debug_prefix, "📋 Hex dump:");
        SBEUtils::print_hex_dump(data, length, debug_prefix + "  ", 64);
    }
    ParseResult result = parse_message(data, length);
    debug_log(debug_prefix, "📋 Parse result: ", (result.success ? "SUCCESS" : "FAILED"));
    debug_log(debug_prefix, "📋 Description: ", result.get_description());
    if (!result.success) {
        debug_log(debug_prefix, "📋 Error: ", result.error_message);
        const auto strings = SBEUtils::extract_readable_strings(data, length, 3);
        if (!strings.empty()) {
            debug_log(debug_prefix, "📋 Readable strings found:");
            for (const auto& str : strings) debug_log(debug_prefix, "  \"", str, "\"");
        }
    }
    return result;
}

std::string MessageParser::get_message_type(const std::uint8_t* data, std::size_t length) {
    if (!data || length < SBEConstants::SBE_HEADER_LENGTH) return "INVALID";
    return SBEUtils::get_message_type_name(rdu16(data + 2), rdu16(data + 4));
}

std::int64_t MessageParser::extract_correlation_id(const std::uint8_t* data, std::size_t length) {
    if (!data || length < SBEConstants::SBE_HEADER_LENGTH + 8) return 0;
    if (rdu16(data + 4) != SBEConstants::CLUSTER_SCHEMA_ID) return 0;
    return rdi64(data + 8);
}

bool MessageParser::is_acknowledgment_for(const std::uint8_t* data, std::size_t length, const std::string& message_id) {
    const ParseResult r = parse_message(data, length);
    if (!r.success || !r.is_acknowledgment()) return false;
    return r.message_id == message_id || r.payload.find(message_id) != std::string::npos ||
           r.headers.find(message_id) != std::string::npos;
}

std::vector<ParseResult> MessageParser::parse_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n) {
    std::vector<ParseResult> out;
    parse_batch(data, rec_off, n, out);
    return out;
}

void MessageParser::parse_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n,
                                std::vector<ParseResult>& out) {
    if (out.size() != n) out.resize(n);
    if (n == 0) return;
    // each chunk's ParseResults are built while the next chunk is on the device
    const ChunkFn fill = [&](const Descriptors& d, size_t a, size_t m) {
        for_ranges(m, 256, [&](size_t x, size_t y) {
            for (size_t i = a + x; i < a + y; ++i) materialize_into(out[i], data + rec_off[i], d, i);
        });
    };
    run_decode(data, rec_off, n, SBE_DEC_PARSE_MESSAGE, &fill);
}

// ---- BatchingParser -------------------------------------------------------------------------
// One batch fills on the caller's thread; handed-off batches queue for the decode thread (its own
// device context), which decodes them in order, and wait, decoded, for the caller's next poll() /
// flush() to deliver them in order.  Options::batches batches are kept (more are made when the
// caller hands off faster than it polls), so a decode overlaps both the next fill and the previous
// delivery: with two batches a 1024-record batch's decode (a serve round trip, ~20 us) could not,
// and each hand-off paid two futex wake-ups (the decode thread's, then the caller's): 23 M rec/s,
// below one CPU thread of the restatement (profiles/r05_host_latency.log).  Waits spin on an
// atomic for a while before they block (states change under the mutex, so a waiter that blocks
// cannot miss the notification).  Handlers run only inside poll() / flush(): on_fragment never
// delivers, so it never throws a handler's exception and never drops the fragment it is given.
struct BatchingParser::Impl {
    using clk = std::chrono::steady_clock;
    enum State : int { kFilling, kDecoding, kReady };
    struct Batch {
        // page-locked (a block of the library's pool, so a new parser reuses the blocks of earlier
        // ones instead of pinning fresh memory): the one-chunk decode reads it in place
        std::shared_ptr<void> blk;
        size_t cap = 0;
        size_t bytes = 0;
        uint8_t* b() const { return static_cast<uint8_t*>(blk.get()); }
        std::vector<uint64_t> off{0};
        ParsedBatch pb;  // the device descriptors; ParseResults are built at delivery
        std::atomic<int> state{kFilling};
        size_t done = 0;  // records already handed to the handler (a throwing handler resumes here)
        clk::time_point first{};
        std::exception_ptr err;
        size_t n() const { return off.size() - 1; }
        void reset() {
            bytes = 0;
            off.resize(1);
            done = 0;
            err = nullptr;
            pb = ParsedBatch();
            state.store(kFilling, std::memory_order_release);
        }
    };
    Handler handler;
    Options opt;
    std::vector<std::unique_ptr<Batch>> all;  // every batch (owner)
    std::vector<Batch*> spare;                // free batches (caller's thread)
    std::deque<Batch*> inflight;              // handed off, oldest first (caller's thread)
    Batch* cur = nullptr;                     // the filling batch
    ParseResult res;  // the result handed to the handler (rewritten in place per record)
    uint64_t n_delivered = 0;
    mutable std::mutex m;
    std::condition_variable cv;
    std::deque<Batch*> todo;                  // the decode thread's queue (under m)
    std::atomic<size_t> todo_n{0};
    std::atomic<bool> stop{false};
    std::thread worker;

    Impl(Handler h, Options o) : handler(std::move(h)), opt(o) {
        if (sbe_device_ready() != 1) fail("no gfx950 device visible");  // as every mirror entry point
        if (opt.max_records == 0) opt.max_records = 1;
        opt.batches = std::max<size_t>(2, std::min<size_t>(opt.batches, 64));
        for (size_t i = 0; i < opt.batches; ++i) spare.push_back(make_batch());
        cur = take();
        worker = std::thread([this] { run(); });
    }
    ~Impl() {
        {
            std::lock_guard<std::mutex> g(m);
            stop.store(true);
        }
        cv.notify_all();
        worker.join();
    }
    Batch* make_batch() {
        all.push_back(std::make_unique<Batch>());
        all.back()->off.reserve(opt.max_records + 1);
        return all.back().get();
    }
    Batch* take() {
        if (spare.empty()) return make_batch();
        Batch* x = spare.back();
        spare.pop_back();
        return x;
    }
    // spin (up to opt.spin) on pred, then block on the condition variable
    template <class Pred>
    void wait_for(Pred pred) {
        if (pred()) return;
        const auto until = clk::now() + opt.spin;
        while (clk::now() < until) {
            for (int k = 0; k < 64; ++k) {
                if (pred()) return;
#if defined(__x86_64__)
                __builtin_ia32_pause();
#endif
            }
        }
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, pred);
    }
    void run() {  // the decode thread: batches in hand-off order
        for (;;) {
            wait_for([&] { return stop.load() || todo_n.load(std::memory_order_acquire) > 0; });
            Batch* x = nullptr;
            {
                std::lock_guard<std::mutex> g(m);
                if (todo.empty()) {
                    if (stop.load()) return;
                    continue;
                }
                x = todo.front();
                todo.pop_front();
                todo_n.fetch_sub(1, std::memory_order_relaxed);
            }
            try {
                x->pb = MessageParser::decode_batch(x->b(), x->off.data(), x->n());
            } catch (...) {
                x->err = std::current_exception();
            }
            {
                std::lock_guard<std::mutex> g(m);
                x->state.store(kReady, std::memory_order_release);
            }
            cv.notify_all();
        }
    }
    void hand_off() {  // the filling batch to the decode thread; filling goes on in a free batch
        Batch* x = cur;
        x->state.store(kDecoding, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> g(m);
            todo.push_back(x);
            todo_n.fetch_add(1, std::memory_order_release);
        }
        cv.notify_all();
        inflight.push_back(x);
        cur = take();
    }
    // the oldest in-flight batch, decoded; a handler that throws leaves it at the front with `done`
    // past the record that threw, so the next call resumes after it
    size_t deliver_front() {
        Batch& x = *inflight.front();
        size_t got = 0;
        if (x.err) {
            std::exception_ptr e = x.err;
            n_delivered += x.n() - x.done;  // the batch's records are consumed by the error
            inflight.pop_front();
            x.reset();
            spare.push_back(&x);
            std::rethrow_exception(e);
        }
        // each result built on this thread into one reused ParseResult right before its handler
        // (the record and the result stay in this core's cache; the reference's handler likewise
        // receives a ParseResult that lives for the call, src/cluster_client.cpp:1185-1190)
        const size_t n = x.n();
        while (x.done < n) {
            const size_t i = x.done++;
            ++n_delivered;
            ++got;
            x.pb.result_into(i, res);
            handler(res);
        }
        inflight.pop_front();
        x.reset();
        spare.push_back(&x);
        return got;
    }
    size_t deliver_ready() {  // in order, up to the first batch still decoding
        size_t got = 0;
        while (!inflight.empty() && inflight.front()->state.load(std::memory_order_acquire) == kReady)
            got += deliver_front();
        return got;
    }
    size_t deliver_all() {
        size_t got = 0;
        while (!inflight.empty()) {
            Batch* x = inflight.front();
            wait_for([&] { return x->state.load(std::memory_order_acquire) == kReady; });
            got += deliver_front();
        }
        return got;
    }
};

BatchingParser::BatchingParser(Handler handler) : BatchingParser(std::move(handler), Options{}) {}
BatchingParser::BatchingParser(Handler handler, Options options)
    : impl_(std::make_unique<Impl>(std::move(handler), options)) {}
BatchingParser::~BatchingParser() {
    for (int k = 0; k < 1000000; ++k) {  // every record given is delivered (a throwing handler's
        try {                            // exception is dropped here: a destructor cannot throw)
            flush();
            return;
        } catch (...) {
        }
    }
}

void BatchingParser::on_fragment(const std::uint8_t* data, std::size_t length) {
    Impl& I = *impl_;
    if (I.cur->n() > 0 && (I.cur->n() + 1 > I.opt.max_records || I.cur->bytes + length > I.opt.max_bytes))
        I.hand_off();
    Impl::Batch& f = *I.cur;
    if (f.bytes + length > f.cap) {  // grow, keeping the bytes already copied
        const size_t want = std::max(f.bytes + length, std::max(I.opt.max_bytes, (size_t)4096));
        std::shared_ptr<void> nb = PinnedPool::get().take(want);
        if (f.bytes) std::memcpy(nb.get(), f.blk.get(), f.bytes);
        f.blk = std::move(nb);
        f.cap = want;
    }
    if (f.n() == 0) f.first = Impl::clk::now();
    if (length) copy_small(f.b() + f.bytes, data, length);
    f.bytes += length;
    f.off.push_back(f.bytes);
}

std::size_t BatchingParser::poll() {
    Impl& I = *impl_;
    // the filling batch goes first when its deadline has passed, so its decode overlaps the
    // delivery of the older ones
    if (I.cur->n() > 0 && Impl::clk::now() - I.cur->first >= I.opt.max_delay) I.hand_off();
    return I.deliver_ready();
}

std::size_t BatchingParser::flush() {
    Impl& I = *impl_;
    if (I.cur->n() > 0) I.hand_off();
    return I.deliver_all();
}

std::size_t BatchingParser::pending() const {
    const Impl& I = *impl_;
    size_t p = I.cur->n();
    for (const Impl::Batch* x : I.inflight) p += x->n() - x->done;
    return p;
}

std::uint64_t BatchingParser::delivered() const { return impl_->n_delivered; }

ParsedBatch MessageParser::decode_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n) {
    ParsedBatch b;
    b.desc_ = run_decode(data, rec_off, n, SBE_DEC_PARSE_MESSAGE);
    b.data_ = data;
    b.rec_off_ = rec_off;
    b.n_ = n;
    return b;
}

ParseResult ParsedBatch::result(std::size_t i) const { return materialize(data_ + rec_off_[i], *desc_, i); }
void ParsedBatch::result_into(std::size_t i, ParseResult& out) const {
    materialize_into(out, data_ + rec_off_[i], *desc_, i);
}
bool ParsedBatch::success(std::size_t i) const { return desc_->status(i) < SBE_ST_ERR_NULL_EMPTY; }
std::uint8_t ParsedBatch::status(std::size_t i) const { return desc_->status(i); }
std::uint16_t ParsedBatch::template_id(std::size_t i) const {
    const uint8_t st = desc_->status(i);
    return (st < SBE_ST_ERR_NULL_EMPTY || st == SBE_ST_ERR_UNKNOWN_TYPE) ? desc_->hdr(i)[1] : 0;
}
std::uint16_t ParsedBatch::schema_id(std::size_t i) const {
    const uint8_t st = desc_->status(i);
    return (st < SBE_ST_ERR_NULL_EMPTY || st == SBE_ST_ERR_UNKNOWN_TYPE) ? desc_->hdr(i)[2] : 0;
}
std::int64_t ParsedBatch::timestamp(std::size_t i) const {
    const uint8_t st = desc_->status(i);
    return (st == SBE_ST_TM || st == SBE_ST_ACK) ? (int64_t)desc_->ts(i) : 0;
}
std::uint64_t ParsedBatch::sequence_number(std::size_t i) const { return desc_->seq(i); }
std::string_view ParsedBatch::view(std::size_t i, int field) const {
    if (field < 0 || field > 4 || desc_->status(i) >= SBE_ST_ERR_NULL_EMPTY) return {};
    return {reinterpret_cast<const char*>(data_ + rec_off_[i]) + desc_->off(i)[field], desc_->len(i)[field]};
}
void ParsedBatch::for_each(const std::function<void(std::size_t, const ParseResult&)>& fn) const {
    const size_t block = 4096;
    std::vector<ParseResult> buf[1];
    auto build = [&](size_t k, std::vector<ParseResult>& v) {
        const size_t a = k * block, m = std::min(n_, a + block) - a;
        v.resize(m);
        for_ranges(m, 256, [&](size_t x, size_t y) {
            for (size_t r = x; r < y; ++r) v[r] = result(a + r);
        });
    };
    const size_t K = (n_ + block - 1) / block;
    for (size_t k = 0; k < K; ++k) {  // a block's ParseResults on the workers, then fn in order
        build(k, buf[0]);
        for (size_t r = 0; r < buf[0].size(); ++r) fn(k * block + r, buf[0][r]);
    }
}

namespace {
std::optional<AckInfo> ack_from(const uint8_t* rec, const Descriptors& d, size_t i) {
    const uint8_t st = d.status(i);
    if (st != SBE_ST_EG_ACK_SIMPLE && st != SBE_ST_EG_ACK) return std::nullopt;
    AckInfo a;
    a.timestamp_nanos = d.ts(i);
    a.simple_control_ack = st == SBE_ST_EG_ACK_SIMPLE;
    if (st == SBE_ST_EG_ACK) {
        const uint32_t* off = d.off(i);
        const uint32_t* len = d.len(i);
        auto v = [&](int k) { return std::string(reinterpret_cast<const char*>(rec) + off[k], len[k]); };
        a.message_id = v(0);
        a.topic = v(1);
        a.correlation_id = v(2);
    }
    return a;
}
}  // namespace

std::optional<AckInfo> decode_ack(const std::uint8_t* data, std::size_t len) {
    if (!data || len < 8) return std::nullopt;  // src/ack_decoder.cpp:30
    const uint64_t off[2] = {0, len};
    auto d = run_decode(data, off, 1, SBE_DEC_ON_EGRESS);
    return ack_from(data, *d, 0);
}

std::optional<LiteRecord> decode_lite(const std::uint8_t* data, std::size_t len) {
    if (!data || len < 8) return std::nullopt;
    const uint64_t off[2] = {0, len};
    auto d = run_decode(data, off, 1, SBE_DEC_LITE);
    if (d->status(0) != SBE_ST_LITE) return std::nullopt;
    LiteRecord r;
    r.template_id = d->hdr(0)[1];
    r.topic_id = d->off(0)[4];
    r.sequence = d->ts(0);
    const int nf = (int)sbe_lite_fields(r.template_id);
    for (int k = 0; k < nf; ++k) r.fields.emplace_back(reinterpret_cast<const char*>(data) + d->off(0)[k], d->len(0)[k]);
    return r;
}

EncodedBatch FragmentReassembler::on_fragments(const std::uint8_t* data, const std::uint64_t* frag_off,
                                               const std::uint8_t* flags, std::size_t n) {
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // serial use of the pipeline's first slot (idle between calls)
    hipStream_t stream = c.batch_stream();
    EncodedBatch b;
    // the accumulator so far goes first as a middle fragment (flags 0): it is appended to exactly
    // as the reference's acc_ would be, or cleared by a BEGIN
    const size_t pre = acc_.empty() ? 0 : 1, nf = n + pre;
    if (nf == 0) {
        b.offsets = HostBytesAccess::make<uint64_t>(1);
        b.offsets[0] = 0;
        return b;
    }
    const uint64_t base = n ? frag_off[0] : 0, body = n ? frag_off[n] - base : 0, total = acc_.size() + body;
    const size_t o_fl = (nf + 1) * 8, o_data = al16(o_fl + nf), stage = o_data + total;
    s.pin.need(stage + 16);
    uint8_t* hp = s.pin.b();
    uint64_t* ho = reinterpret_cast<uint64_t*>(hp);
    uint8_t* hf = hp + o_fl;
    std::memcpy(hp + o_data, acc_.data(), acc_.size());
    if (body) std::memcpy(hp + o_data + acc_.size(), data + base, body);
    ho[0] = 0;
    if (pre) {
        ho[1] = acc_.size();
        hf[0] = 0;
    }
    for (size_t i = 0; i < n; ++i) {
        ho[pre + i + 1] = acc_.size() + (frag_off[i + 1] - base);
        hf[pre + i] = flags[i];
    }
    s.d_in.need(stage + 16);
    const size_t d_off = al16(total), d_cnt = d_off + (nf + 1) * 8, d_ws = al16(d_cnt + 16);
    const size_t wsb = sbe_reassemble_workspace_size(nf);
    s.d_out.need(d_ws + wsb);
    hip_check(hipMemcpyAsync(s.d_in.p, hp, stage, hipMemcpyHostToDevice, stream), "H2D");
    uint8_t* dout = s.d_out.b();
    uint64_t* dmo = reinterpret_cast<uint64_t*>(dout + d_off);
    uint64_t* dcnt = reinterpret_cast<uint64_t*>(dout + d_cnt);
    if (sbe_reassemble_fragments(s.d_in.b() + o_data, reinterpret_cast<const uint64_t*>(s.d_in.p), s.d_in.b() + o_fl, nf,
                                 dout, dmo, dcnt, dout + d_ws, wsb, stream) != SBE_OK)
        fail("sbe_reassemble_fragments");
    c.h_aux.need(16);
    uint64_t* counts = reinterpret_cast<uint64_t*>(c.h_aux.p);
    hip_check(hipMemcpyAsync(counts, dcnt, 16, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const uint64_t m = counts[0], carry = counts[1];
    b.offsets = HostBytesAccess::make<uint64_t>(m + 1);
    b.status = HostBytesAccess::make<uint8_t>(m);
    HostBytesAccess::zero(b.status);
    hip_check(hipMemcpyAsync(b.offsets.data(), dmo, (m + 1) * 8, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const uint64_t msg_bytes = b.offsets[m];
    b.bytes = HostBytesAccess::make((size_t)msg_bytes);
    acc_.resize(carry);
    if (msg_bytes) hip_check(hipMemcpyAsync(b.bytes.data(), dout, msg_bytes, hipMemcpyDeviceToHost, stream), "D2H");
    if (carry) hip_check(hipMemcpyAsync(acc_.data(), dout + msg_bytes, carry, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    return b;
}

EncodedBatch FragmentReassembler::on_term_block(const std::uint8_t* block, std::size_t len, std::size_t start,
                                                std::size_t limit, std::size_t* next) {
    if ((len & 31) || (start & 31) || start > len) throw std::invalid_argument("on_term_block: block and start are multiples of 32");
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // as on_fragments
    hipStream_t stream = c.batch_stream();
    // the accumulator so far goes first as a frame of its own: a middle fragment (flags 0, a data
    // frame), which the walk delivers ahead of the block's and reassembly appends to or clears
    // exactly as on_fragments' leading fragment
    const size_t body = len - start, pre = acc_.empty() ? 0 : ((32 + acc_.size() + 31) & ~(size_t)31);
    const size_t total = pre + body;
    if (total > ((size_t)1 << 30)) throw std::invalid_argument("on_term_block: more than 2^30 bytes");
    const uint64_t lim = pre && limit != ~(size_t)0 ? (uint64_t)limit + 1 : (uint64_t)limit;
    const uint64_t cap = lim < total / 32 ? lim : total / 32;
    s.d_in.need(total + 16);
    if (pre) {
        s.pin.need(pre);
        uint8_t* hp = s.pin.b();
        std::memset(hp, 0, pre);
        const int32_t L = (int32_t)(32 + acc_.size());
        const uint16_t type = 1;
        std::memcpy(hp, &L, 4);
        std::memcpy(hp + 6, &type, 2);
        std::memcpy(hp + 32, acc_.data(), acc_.size());
        hip_check(hipMemcpyAsync(s.d_in.p, hp, pre, hipMemcpyHostToDevice, stream), "H2D");
    }
    if (body) hip_check(hipMemcpyAsync(s.d_in.b() + pre, block + start, body, hipMemcpyHostToDevice, stream), "H2D");
    const size_t o_off = al16(total), o_fl = o_off + (cap + 1) * 8, o_cnt = al16(o_fl + cap), o_ws = o_cnt + 32;
    const size_t wsb = sbe_term_scan_workspace_size(total);
    s.d_out.need(o_ws + wsb + 16);
    uint8_t* dfr = s.d_out.b();
    const sbe_term_out to{reinterpret_cast<uint64_t*>(dfr + o_off), dfr + o_fl, nullptr, reinterpret_cast<uint64_t*>(dfr + o_cnt)};
    if (sbe_term_scan(s.d_in.b(), total, 0, lim, cap, dfr, &to, dfr + o_ws, wsb, stream) != SBE_OK) fail("sbe_term_scan");
    c.h_aux.need(48);
    uint64_t* counts = reinterpret_cast<uint64_t*>(c.h_aux.p);
    hip_check(hipMemcpyAsync(counts, to.counts, 32, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const uint64_t nf = counts[0], payload = counts[2];
    if (next) *next = start + (size_t)counts[1] - pre;  // the accumulator's frame is always consumed (lim >= 1 with it)
    EncodedBatch b;
    if (nf == 0) {
        b.offsets = HostBytesAccess::make<uint64_t>(1);
        b.offsets[0] = 0;
        return b;
    }
    const size_t d_off = al16(payload), d_cnt = d_off + (nf + 1) * 8, d_ws = al16(d_cnt + 16);
    const size_t rwb = sbe_reassemble_workspace_size(nf);
    c.d_aux.need(d_ws + rwb + 16);
    uint8_t* dout = static_cast<uint8_t*>(c.d_aux.p);
    uint64_t* dmo = reinterpret_cast<uint64_t*>(dout + d_off);
    uint64_t* dcnt = reinterpret_cast<uint64_t*>(dout + d_cnt);
    if (sbe_reassemble_fragments(dfr, to.frag_off, to.flags, nf, dout, dmo, dcnt, dout + d_ws, rwb, stream) != SBE_OK)
        fail("sbe_reassemble_fragments");
    hip_check(hipMemcpyAsync(counts + 4, dcnt, 16, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const uint64_t m = counts[4], carry = counts[5];
    b.offsets = HostBytesAccess::make<uint64_t>(m + 1);
    b.status = HostBytesAccess::make<uint8_t>(m);
    HostBytesAccess::zero(b.status);
    hip_check(hipMemcpyAsync(b.offsets.data(), dmo, (m + 1) * 8, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const uint64_t msg_bytes = b.offsets[m];
    b.bytes = HostBytesAccess::make((size_t)msg_bytes);
    acc_.resize(carry);
    if (msg_bytes) hip_check(hipMemcpyAsync(b.bytes.data(), dout, msg_bytes, hipMemcpyDeviceToHost, stream), "D2H");
    if (carry) hip_check(hipMemcpyAsync(acc_.data(), dout + msg_bytes, carry, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    return b;
}

EncodedBatch FragmentReassembler::poll_term_block(const std::uint8_t* block, std::size_t len, std::size_t start,
                                                  std::size_t limit, std::size_t* next) {
    if ((len & 31) || (start & 31) || start > len) throw std::invalid_argument("poll_term_block: block and start are multiples of 32");
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // as on_fragments
    hipStream_t stream = c.batch_stream();
    const size_t body = len - start, carry_in = acc_.size(), bound = carry_in + body;
    if (body > ((size_t)1 << 30) || bound > ((size_t)1 << 31)) throw std::invalid_argument("poll_term_block: more than 2^30 bytes");
    const uint64_t lim = limit == ~(size_t)0 ? ~0ull : (uint64_t)limit;
    const uint64_t cap = lim < body / 32 ? lim : body / 32;
    // the block as it is, the accumulator behind it (the call reads it from there as its carry)
    const size_t i_carry = al16(body);
    s.d_in.need(i_carry + carry_in + 16);
    if (body) hip_check(hipMemcpyAsync(s.d_in.p, block + start, body, hipMemcpyHostToDevice, stream), "H2D");
    if (carry_in) hip_check(hipMemcpyAsync(s.d_in.b() + i_carry, acc_.data(), carry_in, hipMemcpyHostToDevice, stream), "H2D");
    const size_t o_off = al16(bound), o_cnt = o_off + (cap + 1) * 8, o_ws = al16(o_cnt + 48);
    const size_t wsb = sbe_term_poll_workspace_size(body, cap);
    s.d_out.need(o_ws + wsb + 16);
    uint8_t* dout = s.d_out.b();
    const sbe_term_poll_out po{reinterpret_cast<uint64_t*>(dout + o_off), reinterpret_cast<uint64_t*>(dout + o_cnt)};
    if (sbe_term_poll(s.d_in.b(), body, 0, lim, cap, carry_in ? s.d_in.b() + i_carry : nullptr, carry_in, dout, bound, &po,
                      dout + o_ws, wsb, stream) != SBE_OK)
        fail("sbe_term_poll");
    c.h_aux.need(48);
    uint64_t* counts = reinterpret_cast<uint64_t*>(c.h_aux.p);
    hip_check(hipMemcpyAsync(counts, po.counts, 48, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");  // the call's one wait: the rest are the downloads
    if (next) *next = start + (size_t)counts[1];
    const uint64_t m = counts[4], carry = counts[5];
    EncodedBatch b;
    b.offsets = HostBytesAccess::make<uint64_t>(m + 1);
    b.offsets[0] = 0;
    if (counts[0] == 0) return b;  // no fragment: nothing delivered, the accumulator as it was
    b.status = HostBytesAccess::make<uint8_t>(m);
    HostBytesAccess::zero(b.status);
    hip_check(hipMemcpyAsync(b.offsets.data(), po.msg_off, (m + 1) * 8, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const uint64_t msg_bytes = b.offsets[m];
    b.bytes = HostBytesAccess::make((size_t)msg_bytes);
    acc_.resize(carry);
    if (msg_bytes) hip_check(hipMemcpyAsync(b.bytes.data(), dout, msg_bytes, hipMemcpyDeviceToHost, stream), "D2H");
    if (carry) hip_check(hipMemcpyAsync(acc_.data(), dout + msg_bytes, carry, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    return b;
}

TermAppendResult TermAppender::append_batch(const EncodedBatch& batch, std::size_t first_record, std::uint8_t* block,
                                            std::size_t len, std::size_t start, const TermAppendOptions& options) {
    const size_t total = batch.offsets.size() ? batch.offsets.size() - 1 : 0;
    if (first_record > total) throw std::invalid_argument("append_batch: first_record behind the batch");
    // the offsets index the batch's bytes as they are
    return append(batch.bytes.data(), batch.bytes.size(), batch.offsets.data() + first_record, total - first_record, block, len,
                  start, options);
}

TermAppendResult TermAppender::append(const std::uint8_t* data, std::size_t nbytes, const std::uint64_t* rec_off, std::size_t n,
                                      std::uint8_t* block, std::size_t len, std::size_t start, const TermAppendOptions& options) {
    options.check(len, start);
    TermAppendResult r;
    r.next = start;
    r.stop = SBE_TERM_APPEND_END;
    if (n == 0) return r;
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // as on_fragments
    hipStream_t stream = c.batch_stream();
    // device input: the offsets of the records, then the bytes they index
    const size_t o_data = al16((n + 1) * 8);
    s.d_in.need(o_data + nbytes + 16);
    hip_check(hipMemcpyAsync(s.d_in.p, rec_off, (n + 1) * 8, hipMemcpyHostToDevice, stream), "H2D");
    if (nbytes) hip_check(hipMemcpyAsync(s.d_in.b() + o_data, data, nbytes, hipMemcpyHostToDevice, stream), "H2D");
    // device output: the block, the tails, counts, the workspace
    const size_t o_tail = al16(len), o_cnt = o_tail + n * 8, o_ws = al16(o_cnt + 32);
    const size_t wsb = sbe_term_append_workspace_size(n);
    s.d_out.need(o_ws + wsb + 16);
    uint8_t* d = s.d_out.b();
    const sbe_term_header h{options.header.session_id, options.header.stream_id, options.header.term_id,
                            options.header.term_offset_base, options.header.version};
    const sbe_term_append_out o{reinterpret_cast<uint64_t*>(d + o_tail), reinterpret_cast<uint64_t*>(d + o_cnt)};
    if (sbe_term_append(s.d_in.b() + o_data, nbytes, reinterpret_cast<const uint64_t*>(s.d_in.p), n, d, len, start, options.limit,
                        options.mtu, options.effective_max_message_length(len), &h, &o, d + o_ws, wsb, stream) != SBE_OK)
        fail("sbe_term_append");
    c.h_aux.need(32);
    uint64_t* counts = reinterpret_cast<uint64_t*>(c.h_aux.p);
    hip_check(hipMemcpyAsync(counts, o.counts, 32, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    r.appended = (size_t)counts[0];
    r.next = counts[1];
    r.stop = (uint32_t)counts[3];
    r.rec_tail.resize(r.appended);
    if (r.appended) hip_check(hipMemcpyAsync(r.rec_tail.data(), o.rec_tail, r.appended * 8, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    // what the call wrote: the frames, and of a padding frame its header
    const uint64_t data_end = r.appended ? r.rec_tail.back() : start;
    const uint64_t end = data_end + (r.stop == SBE_TERM_APPEND_TRIPPED && data_end < len ? 32 : 0);
    if (end > start) hip_check(hipMemcpyAsync(block + start, d + start, end - start, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    return r;
}

EgressCommitter::EgressCommitter(std::string client_id, std::string fallback_topic)
    : client_id_(std::move(client_id)), fallback_(std::move(fallback_topic)) {
    if (fallback_.size() > SBE_COMMIT_TABLE_BYTES) throw std::length_error("EgressCommitter: fallback topic too long");
}

void EgressCommitter::set_message_identifier(const std::string& topic, const std::string& identifier) {
    if (!identifiers_.count(topic)) {
        size_t bytes = fallback_.size() + topic.size();
        for (const auto& kv : identifiers_) bytes += kv.first.size();
        if (identifiers_.size() + 2 > SBE_COMMIT_MAX_TOPICS || bytes > SBE_COMMIT_TABLE_BYTES)
            throw std::length_error("EgressCommitter: the topic table holds 64 topics and 4096 bytes");
    }
    identifiers_[topic] = identifier;
}

EgressStepResult EgressCommitter::poll_commit_append(const std::uint8_t* block, std::size_t len, std::size_t start,
                                                     std::uint8_t* ingress, std::size_t ingress_len, std::size_t ingress_start,
                                                     const EgressStepOptions& options, EncodedBatch* messages) {
    if ((len & 31) || (start & 31) || start > len)
        throw std::invalid_argument("poll_commit_append: block and start are multiples of 32");
    options.append.check(ingress_len, ingress_start);
    const size_t body = len - start, carry_in = acc_.size(), bound = carry_in + body;
    if (body > ((size_t)1 << 30) || bound > ((size_t)1 << 31)) throw std::invalid_argument("poll_commit_append: more than 2^30 bytes");
    if (client_id_.size() > SBE_COMMIT_TABLE_BYTES) throw std::length_error("EgressCommitter: the default identifier holds 4096 bytes");
    // the tables of AutoCommitter::run: the fallback topic, then the topics with an identifier
    std::vector<const std::string*> table{&fallback_};
    for (const auto& kv : identifiers_) table.push_back(&kv.first);
    const uint32_t k = (uint32_t)table.size();
    auto ident = [&](const std::string& t) -> const std::string& {
        auto it = identifiers_.find(t);
        return it == identifiers_.end() ? client_id_ : it->second;
    };
    size_t ident_bytes = 0, ident_max = client_id_.size();
    for (const std::string* t : table) {
        ident_bytes += ident(*t).size();
        ident_max = std::max(ident_max, ident(*t).size());
    }
    if (ident_bytes > SBE_COMMIT_TABLE_BYTES) throw std::length_error("EgressCommitter: the identifier table holds 4096 bytes");
    const uint64_t now_ns = options.clock ? options.clock() : now_nanos_sys();
    const uint64_t uuid_ns = options.clock ? options.clock() : now_nanos_sys();

    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // as poll_term_block
    hipStream_t stream = c.batch_stream();
    const uint64_t lim = options.limit == ~(size_t)0 ? ~0ull : (uint64_t)options.limit;
    const size_t cap = (size_t)(lim < body / 32 ? lim : body / 32);  // fragments, and so messages, at most
    // staged tables: topic arena and offsets, topic ids, identifier arena and offsets, client_id
    const size_t t_to = SBE_COMMIT_TABLE_BYTES, t_tid = t_to + al16(4 * (SBE_COMMIT_MAX_TOPICS + 1)),
                 t_ia = t_tid + al16(4 * SBE_COMMIT_MAX_TOPICS), t_io = t_ia + SBE_COMMIT_TABLE_BYTES,
                 t_di = t_io + al16(4 * (SBE_COMMIT_MAX_TOPICS + 1)), tables = t_di + SBE_COMMIT_TABLE_BYTES;
    s.pin.need(tables);
    uint8_t* hp = s.pin.b();
    std::memset(hp, 0, tables);
    uint32_t* to = reinterpret_cast<uint32_t*>(hp + t_to);
    uint32_t* tid = reinterpret_cast<uint32_t*>(hp + t_tid);
    uint32_t* io = reinterpret_cast<uint32_t*>(hp + t_io);
    for (uint32_t j = 0; j < k; ++j) {
        const std::string& id = ident(*table[j]);
        std::memcpy(hp + to[j], table[j]->data(), table[j]->size());
        to[j + 1] = to[j] + (uint32_t)table[j]->size();
        tid[j] = CommitManager::topic_to_id(*table[j]);
        std::memcpy(hp + t_ia + io[j], id.data(), id.size());
        io[j + 1] = io[j] + (uint32_t)id.size();
    }
    std::memcpy(hp + t_di, client_id_.data(), client_id_.size());
    // device input: the block as it is, the accumulator (the poll's carry), the tables
    const size_t i_carry = al16(body), i_tab = al16(i_carry + carry_in);
    s.d_in.need(i_tab + tables + 16);
    uint8_t* di = s.d_in.b();
    if (body) hip_check(hipMemcpyAsync(di, block + start, body, hipMemcpyHostToDevice, stream), "H2D");
    if (carry_in) hip_check(hipMemcpyAsync(di + i_carry, acc_.data(), carry_in, hipMemcpyHostToDevice, stream), "H2D");
    hip_check(hipMemcpyAsync(di + i_tab, hp, tables, hipMemcpyHostToDevice, stream), "H2D");
    // device output, every per-record array sized by the capacity
    const size_t n = cap, n1 = n ? n : 1;
    const size_t frames_cap = (size_t)sbe_commit_fallback_output_bound(n, bound + n * ident_max, 1);
    const size_t w_poll = sbe_term_poll_workspace_size(body, cap), w_emit = sbe_commit_emit_workspace_size(n),
                 w_app = sbe_term_append_workspace_size(n);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t o = at;
        at = al16(at + bytes);
        return o;
    };
    const size_t o_out = take(bound + 16), o_moff = take(8 * (n + 1)), o_pcnt = take(48), o_st = take(n1), o_fl = take(n1),
                 o_hdr = take(8 * n1), o_ts = take(8 * n1), o_vo = take(20 * n1), o_vl = take(20 * n1), o_seq = take(8 * n1),
                 p_cm = take(n1), p_src = take(n1), p_kind = take(n1), p_off = take(4 * n1), p_len = take(4 * n1),
                 p_idx = take(4 * n1), p_last = take(8 * SBE_COMMIT_MAX_TOPICS), p_cnt = take(8 * (SBE_COMMIT_MAX_TOPICS + 2)),
                 e_st = take(n1), e_off = take(8 * (n + 1)), e_idx = take(8 * n1), e_tot = take(32), a_tail = take(8 * n1),
                 a_cnt = take(32), o_wp = take(w_poll + 16), o_we = take(w_emit + 16), o_wa = take(w_app + 16),
                 o_frames = take(frames_cap + 16), o_blk = take(ingress_len + 16);
    s.d_out.need(at);
    uint8_t* d = s.d_out.b();
    auto u64p = [&](size_t o) { return reinterpret_cast<uint64_t*>(d + o); };
    auto u32p = [&](size_t o) { return reinterpret_cast<uint32_t*>(d + o); };
    const sbe_term_poll_out po{u64p(o_moff), u64p(o_pcnt)};
    if (sbe_term_poll(di, body, 0, lim, cap, carry_in ? di + i_carry : nullptr, carry_in, d + o_out, bound, &po, d + o_wp, w_poll,
                      stream) != SBE_OK)
        fail("sbe_term_poll");
    const uint64_t* n_dev = po.counts + 4;  // the message count stays where the poll left it
    const sbe_decoded dec{d + o_st, d + o_fl, reinterpret_cast<uint16_t*>(d + o_hdr), u64p(o_ts), u32p(o_vo), u32p(o_vl), u64p(o_seq)};
    const sbe_commit_out plan{d + p_cm, d + p_src, d + p_kind, u32p(p_off), u32p(p_len), u32p(p_idx), u64p(p_last), u64p(p_cnt)};
    const sbe_commit_fallback fb{di + i_tab, reinterpret_cast<const uint32_t*>(di + i_tab + t_to), di + i_tab + t_di,
                                 (uint32_t)client_id_.size(), now_ns, uuid_ns};
    const sbe_commit_emit_out res{u64p(e_off), d + e_st, u64p(e_idx), u64p(e_tot)};
    const sbe_term_header h{options.append.header.session_id, options.append.header.stream_id, options.append.header.term_id,
                            options.append.header.term_offset_base, options.append.header.version};
    const sbe_term_append_out ao{u64p(a_tail), u64p(a_cnt)};
    const bool ok =
        sbe_decode_batch_counted(d + o_out, po.msg_off, n_dev, n, 0, SBE_DEC_PARSE_MESSAGE, &dec, stream) == SBE_OK &&
        sbe_classify_commits_counted(d + o_out, po.msg_off, n_dev, n, &dec, di + i_tab, fb.topic_off, k, &plan, nullptr, 0,
                                     stream) == SBE_OK &&
        sbe_emit_commit_offsets_counted(d + o_out, po.msg_off, n_dev, n, &dec, &plan,
                                        reinterpret_cast<const uint32_t*>(di + i_tab + t_tid), di + i_tab + t_ia,
                                        reinterpret_cast<const uint32_t*>(di + i_tab + t_io), k, nullptr, 0, 1,
                                        options.leadership_term_id, options.cluster_session_id, d + o_frames, frames_cap, &res,
                                        d + o_we, w_emit, stream, &fb) == SBE_OK &&
        sbe_term_append_counted(d + o_frames, frames_cap, res.out_off, res.emit_idx, res.totals, n, d + o_blk, ingress_len,
                                ingress_start, options.append.limit, options.append.mtu,
                                options.append.effective_max_message_length(ingress_len), &h, &ao, d + o_wa, w_app,
                                stream) == SBE_OK;
    if (!ok) {
        c.abort_all();
        fail("poll_commit_append");
    }
    c.h_aux.need(128);
    uint64_t* hc = reinterpret_cast<uint64_t*>(c.h_aux.p);  // poll counts [6], totals [3] at 6, append counts [4] at 10
    hip_check(hipMemcpyAsync(hc, po.counts, 48, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipMemcpyAsync(hc + 6, res.totals, 24, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipMemcpyAsync(hc + 10, ao.counts, 32, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");  // the one wait for the kernels: the two below are for downloads
    EgressStepResult r;
    std::memcpy(r.poll_counts, hc, 48);
    r.next = start + (size_t)hc[1];
    const size_t m = (size_t)hc[4], carry = (size_t)hc[5];
    r.messages = m;
    r.frames = hc[6];
    r.frame_bytes = hc[7];
    r.appended.appended = (size_t)hc[10];
    r.appended.next = hc[11];
    r.appended.stop = (uint32_t)hc[13];
    if (hc[0] == 0) {  // no fragment: nothing delivered, the accumulator as it was
        if (messages) {
            *messages = EncodedBatch();
            messages->offsets = HostBytesAccess::make<uint64_t>(1);
            messages->offsets[0] = 0;
        }
        return r;
    }
    std::vector<uint8_t> st(m);
    std::vector<uint64_t> moff(m + 1), fidx((size_t)r.frames);
    r.appended.rec_tail.resize(r.appended.appended);
    hip_check(hipMemcpyAsync(moff.data(), po.msg_off, 8 * (m + 1), hipMemcpyDeviceToHost, stream), "D2H");
    if (m) hip_check(hipMemcpyAsync(st.data(), res.status, m, hipMemcpyDeviceToHost, stream), "D2H");
    if (r.frames) hip_check(hipMemcpyAsync(fidx.data(), res.emit_idx, 8 * fidx.size(), hipMemcpyDeviceToHost, stream), "D2H");
    if (r.appended.appended)
        hip_check(hipMemcpyAsync(r.appended.rec_tail.data(), ao.rec_tail, 8 * r.appended.appended, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    const size_t msg_bytes = (size_t)moff[m];
    acc_.resize(carry);
    if (carry) hip_check(hipMemcpyAsync(acc_.data(), d + o_out + msg_bytes, carry, hipMemcpyDeviceToHost, stream), "D2H");
    if (messages) {
        *messages = EncodedBatch();
        messages->offsets = HostBytesAccess::make<uint64_t>(m + 1);
        std::memcpy(messages->offsets.data(), moff.data(), 8 * (m + 1));
        messages->status = HostBytesAccess::make<uint8_t>(m);
        HostBytesAccess::zero(messages->status);
        messages->bytes = HostBytesAccess::make(msg_bytes);
        if (msg_bytes) hip_check(hipMemcpyAsync(messages->bytes.data(), d + o_out, msg_bytes, hipMemcpyDeviceToHost, stream), "D2H");
    }
    // what the append wrote: the frames, and of a padding frame its header
    const uint64_t data_end = r.appended.appended ? r.appended.rec_tail.back() : ingress_start;
    const uint64_t end = data_end + (r.appended.stop == SBE_TERM_APPEND_TRIPPED && data_end < ingress_len ? 32 : 0);
    if (end > ingress_start)
        hip_check(hipMemcpyAsync(ingress + ingress_start, d + o_blk + ingress_start, end - ingress_start, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "sync");
    r.frame_record.assign(fidx.begin(), fidx.end());
    for (size_t i = 0; i < m; ++i) {
        if (st[i] == SBE_CE_HOST) r.host.push_back(i);
        else if (st[i] == SBE_CE_E109_MESSAGE_ID) r.too_long.push_back(i);
        else if (st[i] == SBE_CE_E100_FALLBACK) r.fallback_e100.push_back(i);
    }
    return r;
}

MessageHandler::MessageHandler() = default;
MessageHandler::~MessageHandler() = default;

void MessageHandler::handleMessage(const ParseResult& result) {
    // src/message_handler.cpp:10-16: std::cout << std::string, so every byte of the string is
    // written (embedded NULs included), then std::endl
    if (result.success)
        std::cout << "[MessageHandler] Handled message: " << result.message_type << std::endl;
    else
        std::cout << "[MessageHandler] Failed to handle message: " << result.error_message << std::endl;
}

void MessageHandler::on_egress(const std::uint8_t* data, std::size_t len) {
    if (len < 8) return;
    const uint64_t off[2] = {0, len};
    on_egress_batch(data, off, 1);
}

void MessageHandler::on_egress_batch(const std::uint8_t* data, const std::uint64_t* rec_off, std::size_t n) {
    auto d = run_decode(data, rec_off, n, SBE_DEC_ON_EGRESS);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* rec = data + rec_off[i];
        switch (d->status(i)) {
            case SBE_ST_EG_ACK_SIMPLE:
            case SBE_ST_EG_ACK:
                if (ack_cb_) ack_cb_(*ack_from(rec, *d, i));
                break;
            case SBE_ST_EG_TM:
                if (tm_cb_) {
                    const uint32_t* off = d->off(i);
                    const uint32_t* len = d->len(i);
                    auto v = [&](int k) { return std::string_view(reinterpret_cast<const char*>(rec) + off[k], len[k]); };
                    tm_cb_(v(0), v(1), v(2), v(3), v(4));
                }
                break;
            case SBE_ST_EG_THROW_E100: throw std::runtime_error("buffer too short [E100]");
            default: break;  // SBE_ST_EG_NONE
        }
    }
}

// ======================================================================================
// AckCorrelator
// ======================================================================================
namespace {
// One sbe_inflight_* table in device memory that grows by rehash.
struct InfTable {
    DevBuf mem;
    uint64_t cap = 0, used_bound = 0, rehashes = 0;
    uint32_t tag_bits = 0;

    static uint8_t* aligned(const DevBuf& b) {
        return reinterpret_cast<uint8_t*>((reinterpret_cast<uintptr_t>(b.p) + 63) & ~uintptr_t(63));
    }
    uint8_t* p() const { return aligned(mem); }
    void init(uint64_t c, uint32_t tb, hipStream_t s) {
        cap = c;
        tag_bits = tb;
        mem.need(sbe_inflight_table_size(c) + 64);
        if (sbe_inflight_init(p(), sbe_inflight_table_size(c), c, tb, s) != SBE_OK) fail("sbe_inflight_init");
    }
    // capacity, live, used, tag bits, answered
    void header(uint64_t h[5], hipStream_t s) const {
        hip_check(hipMemcpyAsync(h, p(), 40, hipMemcpyDeviceToHost, s), "D2H");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
    // room for n more inserts below half the capacity, by rehash when needed
    void reserve(uint64_t n, hipStream_t s) {
        if (used_bound + n <= cap / 2) return;
        uint64_t h[5];
        header(h, s);
        used_bound = h[2];
        if (used_bound + n <= cap / 2) return;
        uint64_t ncap = cap;
        while (h[1] + n > ncap / 2) ncap *= 2;
        if (ncap > (1ull << 31)) throw std::runtime_error("sbecodec: the in-flight table cannot grow past 2^31 slots");
        DevBuf fresh;
        fresh.need(sbe_inflight_table_size(ncap) + 64);
        uint8_t* dst = aligned(fresh);
        if (sbe_inflight_init(dst, sbe_inflight_table_size(ncap), ncap, tag_bits, s) != SBE_OK) fail("sbe_inflight_init");
        if (sbe_inflight_rehash(p(), dst, s) != SBE_OK) fail("sbe_inflight_rehash");
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
        std::swap(mem.p, fresh.p);
        std::swap(mem.cap, fresh.cap);
        cap = ncap;
        used_bound = h[1];
        ++rehashes;
    }
};
}  // namespace

struct AckCorrelator::Impl {
    hipStream_t stream = nullptr;
    InfTable table;
    DevBuf in, out;  // staged inputs; descriptors / results / workspace
    std::unordered_map<std::string, uint64_t> long_keys;  // keys the table cannot hold
    std::vector<uint8_t> stage;

    uint8_t* tbl() const { return table.p(); }
    static size_t al(size_t v) { return (v + 63) & ~size_t(63); }
    void sync() { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); }
};

AckCorrelator::AckCorrelator(std::uint64_t initial_capacity, std::uint32_t tag_bits) : impl_(new Impl) {
    Impl& m = *impl_;
    const size_t bytes = sbe_inflight_table_size(initial_capacity);
    if (!bytes || tag_bits > 30) throw std::invalid_argument("AckCorrelator: capacity must be a power of two in 64 .. 2^31");
    hip_check(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking), "hipStreamCreate");
    m.table.init(initial_capacity, tag_bits, m.stream);
    m.sync();
}

AckCorrelator::~AckCorrelator() {
    if (impl_->stream) {
        (void)hipStreamSynchronize(impl_->stream);
        (void)hipStreamDestroy(impl_->stream);
    }
}

std::uint64_t AckCorrelator::capacity() const { return impl_->table.cap; }
std::uint64_t AckCorrelator::rehashes() const { return impl_->table.rehashes; }
std::size_t AckCorrelator::size() const {
    uint64_t h[5];
    impl_->table.header(h, impl_->stream);
    return (size_t)h[1] + impl_->long_keys.size();
}

void AckCorrelator::remember_outgoing(const std::string& uuid, std::uint64_t ts_nanos) {
    remember_batch({uuid}, {ts_nanos});
}

void AckCorrelator::remember_batch(const std::vector<std::string>& uuids, const std::vector<std::uint64_t>& ts_nanos) {
    if (uuids.size() != ts_nanos.size()) throw std::invalid_argument("AckCorrelator::remember_batch: sizes differ");
    Impl& m = *impl_;
    // staged: ts [k] u64, key_off [k] u32, key_len [k] u32, key bytes
    size_t k = 0, bytes = 0;
    for (const std::string& u : uuids) {
        if (u.size() <= SBE_INFLIGHT_KEY_MAX) {
            ++k;
            bytes += u.size();
        }
    }
    const size_t o_off = 8 * k, o_len = o_off + 4 * k, o_key = o_len + 4 * k, total = o_key + bytes + 16;
    m.stage.resize(total);
    uint64_t* ts = reinterpret_cast<uint64_t*>(m.stage.data());
    uint32_t* off = reinterpret_cast<uint32_t*>(m.stage.data() + o_off);
    uint32_t* len = reinterpret_cast<uint32_t*>(m.stage.data() + o_len);
    size_t j = 0, pos = 0;
    for (size_t i = 0; i < uuids.size(); ++i) {
        const std::string& u = uuids[i];
        if (u.size() > SBE_INFLIGHT_KEY_MAX) {
            m.long_keys.emplace(u, ts_nanos[i]);  // inflight_.emplace(uuid, ts_nanos)
            continue;
        }
        ts[j] = ts_nanos[i];
        off[j] = (uint32_t)pos;
        len[j] = (uint32_t)u.size();
        std::memcpy(m.stage.data() + o_key + pos, u.data(), u.size());
        pos += u.size();
        ++j;
    }
    if (!k) return;
    if (bytes > 0xffffffffull) throw std::invalid_argument("AckCorrelator::remember_batch: more than 4 GiB of keys");
    m.table.reserve(k, m.stream);
    const size_t wsb = sbe_inflight_workspace_size(k);
    m.in.need(total);
    m.out.need(wsb);
    hip_check(hipMemcpyAsync(m.in.p, m.stage.data(), total, hipMemcpyHostToDevice, m.stream), "H2D");
    // a stored ts of 0 stays 0: ts_default 0 (the reference stores what it is given)
    if (sbe_inflight_remember(m.tbl(), m.in.b() + o_key, reinterpret_cast<const uint32_t*>(m.in.b() + o_off),
                              reinterpret_cast<const uint32_t*>(m.in.b() + o_len), 1,
                              reinterpret_cast<const uint64_t*>(m.in.p), 0, nullptr, k, nullptr, m.out.p, wsb,
                              m.stream) != SBE_OK)
        fail("sbe_inflight_remember");
    m.sync();  // the staging buffer is reused by the next call
    m.table.used_bound += k;
}

namespace {
// Device layout of a match call's descriptors and results behind `base` (64-B aligned pieces).
struct AckLayout {
    size_t status, flags, hdr, ts, voff, vlen, code, base_ns, counts, ws, total;
    explicit AckLayout(size_t n) {
        auto al = [](size_t v) { return (v + 63) & ~size_t(63); };
        size_t p = 0;
        status = p, p = al(p + n);
        flags = p, p = al(p + n);
        hdr = p, p = al(p + 8 * n);
        ts = p, p = al(p + 8 * n);
        voff = p, p = al(p + 20 * n);
        vlen = p, p = al(p + 20 * n);
        code = p, p = al(p + n);
        base_ns = p, p = al(p + 8 * n);
        counts = p, p = al(p + 16);
        ws = p, p = al(p + sbe_inflight_workspace_size(n));
        total = p;
    }
};
}  // namespace

AckMatch AckCorrelator::on_ack(const AckInfo& ack, std::uint64_t now_ns) {
    Impl& m = *impl_;
    auto miss = [&] { return AckMatch{false, (int64_t)now_ns - (int64_t)ack.timestamp_nanos}; };
    if (ack.message_id.empty()) return miss();
    if (ack.message_id.size() > SBE_INFLIGHT_KEY_MAX) {
        auto it = m.long_keys.find(ack.message_id);
        if (it == m.long_keys.end()) return miss();
        const uint64_t send_ns = it->second;
        m.long_keys.erase(it);
        return AckMatch{true, (int64_t)now_ns - (int64_t)send_ns};
    }
    // a one-record batch whose descriptor is written here instead of decoded: the id is the record.
    // staged: the id bytes | rec_off [2] | the descriptor arrays of the layout (outputs follow them)
    const AckLayout L(1);
    const size_t idb = ack.message_id.size(), o_rec = 64, o_desc = 128;
    m.stage.assign(o_desc + L.code, 0);
    std::memcpy(m.stage.data(), ack.message_id.data(), idb);
    const uint64_t rec[2] = {0, idb};
    std::memcpy(m.stage.data() + o_rec, rec, 16);
    m.stage[o_desc + L.status] = SBE_ST_EG_ACK;
    std::memcpy(m.stage.data() + o_desc + L.ts, &ack.timestamp_nanos, 8);
    const uint32_t vl = (uint32_t)idb;
    std::memcpy(m.stage.data() + o_desc + L.vlen, &vl, 4);
    m.in.need(o_desc + L.total);
    hip_check(hipMemcpyAsync(m.in.p, m.stage.data(), o_desc + L.code, hipMemcpyHostToDevice, m.stream), "H2D");
    uint8_t* d = m.in.b() + o_desc;
    sbe_decoded dec{d + L.status, d + L.flags, reinterpret_cast<uint16_t*>(d + L.hdr), reinterpret_cast<uint64_t*>(d + L.ts),
                    reinterpret_cast<uint32_t*>(d + L.voff), reinterpret_cast<uint32_t*>(d + L.vlen), nullptr};
    sbe_ack_out out{d + L.code, reinterpret_cast<uint64_t*>(d + L.base_ns), nullptr};
    if (sbe_inflight_match_acks(m.tbl(), m.in.b(), reinterpret_cast<const uint64_t*>(m.in.b() + o_rec), 1, &dec, &out,
                                d + L.ws, sbe_inflight_workspace_size(1), m.stream) != SBE_OK)
        fail("sbe_inflight_match_acks");
    uint8_t code = 0;
    uint64_t base = 0;
    hip_check(hipMemcpyAsync(&code, d + L.code, 1, hipMemcpyDeviceToHost, m.stream), "D2H");
    hip_check(hipMemcpyAsync(&base, d + L.base_ns, 8, hipMemcpyDeviceToHost, m.stream), "D2H");
    m.sync();
    return AckMatch{code == SBE_ACK_MATCHED, (int64_t)now_ns - (int64_t)base};
}

std::vector<AckMatch> AckCorrelator::on_egress_batch(const std::uint8_t* data, const std::uint64_t* rec_off,
                                                     std::size_t n, std::uint64_t now_ns) {
    std::vector<AckMatch> res;
    if (!n) return res;
    Impl& m = *impl_;
    const AckLayout L(n);
    const uint64_t base0 = rec_off[0], bytes = rec_off[n] - base0;
    // staged: rec_off rebased to 0 [n + 1], then the record bytes (16-B aligned)
    const size_t o_data = Impl::al(8 * (n + 1)), total_in = o_data + bytes + 16;
    m.stage.resize(total_in);
    uint64_t* ro = reinterpret_cast<uint64_t*>(m.stage.data());
    for (size_t i = 0; i <= n; ++i) ro[i] = rec_off[i] - base0;
    if (bytes) std::memcpy(m.stage.data() + o_data, data + base0, bytes);
    m.in.need(total_in);
    m.out.need(L.total);
    hip_check(hipMemcpyAsync(m.in.p, m.stage.data(), total_in, hipMemcpyHostToDevice, m.stream), "H2D");
    uint8_t* d = m.out.b();
    sbe_decoded dec{d + L.status, d + L.flags, reinterpret_cast<uint16_t*>(d + L.hdr), reinterpret_cast<uint64_t*>(d + L.ts),
                    reinterpret_cast<uint32_t*>(d + L.voff), reinterpret_cast<uint32_t*>(d + L.vlen), nullptr};
    const uint64_t* d_ro = reinterpret_cast<const uint64_t*>(m.in.p);
    if (sbe_decode_batch_sized(m.in.b() + o_data, d_ro, n, bytes, SBE_DEC_ON_EGRESS, &dec, m.stream) != SBE_OK)
        fail("sbe_decode_batch");
    sbe_ack_out out{d + L.code, reinterpret_cast<uint64_t*>(d + L.base_ns), nullptr};
    if (sbe_inflight_match_acks(m.tbl(), m.in.b() + o_data, d_ro, n, &dec, &out, d + L.ws, sbe_inflight_workspace_size(n),
                                m.stream) != SBE_OK)
        fail("sbe_inflight_match_acks");
    std::vector<uint8_t> code(n);
    std::vector<uint64_t> base(n);
    hip_check(hipMemcpyAsync(code.data(), d + L.code, n, hipMemcpyDeviceToHost, m.stream), "D2H");
    hip_check(hipMemcpyAsync(base.data(), d + L.base_ns, 8 * n, hipMemcpyDeviceToHost, m.stream), "D2H");
    m.sync();
    // ids the table cannot hold: their views come back too, and the host map answers
    std::vector<uint32_t> voff, vlen;
    if (std::find(code.begin(), code.end(), (uint8_t)SBE_ACK_LONG_ID) != code.end()) {
        voff.resize(5 * n);
        vlen.resize(5 * n);
        hip_check(hipMemcpyAsync(voff.data(), d + L.voff, 20 * n, hipMemcpyDeviceToHost, m.stream), "D2H");
        hip_check(hipMemcpyAsync(vlen.data(), d + L.vlen, 20 * n, hipMemcpyDeviceToHost, m.stream), "D2H");
        m.sync();
    }
    for (size_t i = 0; i < n; ++i) {
        if (code[i] == SBE_ACK_NONE) continue;
        bool matched = code[i] == SBE_ACK_MATCHED;
        uint64_t b = base[i];
        if (code[i] == SBE_ACK_LONG_ID) {
            auto it = m.long_keys.find(std::string(reinterpret_cast<const char*>(data) + rec_off[i] + voff[5 * i], vlen[5 * i]));
            if (it != m.long_keys.end()) {
                matched = true;
                b = it->second;
                m.long_keys.erase(it);
            }
        }
        res.push_back(AckMatch{matched, (int64_t)now_ns - (int64_t)b});
    }
    return res;
}

std::size_t offer_batch(const EncodedBatch& batch, const OfferFn& offer) {
    const size_t n = batch.offsets.empty() ? 0 : batch.offsets.size() - 1;
    for (size_t i = 0; i < n; ++i) {
        if (batch.offsets[i + 1] == batch.offsets[i]) continue;  // failed record (status != 0)
        if (!offer(batch.bytes.data() + batch.offsets[i], batch.offsets[i + 1] - batch.offsets[i])) return i;
    }
    return n;
}

// ======================================================================================
// JSON members by path (sbe_json_extract_batch): ParsedBatch::extract, extract_json_documents,
// extract_order_ids (examples/pubsub_reconnect_test.cpp:576-620), CommitManager::parse_commit_offset
// (src/commit_manager.cpp:177-195)
JsonPath::JsonPath(const std::string& dotted) {
    size_t a = 0;
    for (;;) {
        const size_t b = dotted.find('.', a);
        names.push_back(dotted.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
}

struct JsonExtractAccess {
    // One launch over staged records.  d: the decode descriptors (null: bare documents, view 0);
    // piece(i): record i's bytes; out.base_ is the caller's to fill.  order_select (with d, and no
    // select of the caller's): the mask is sbe_order_select's, computed on the device in front of
    // the extract, on the same stream.
    template <class Piece>
    static void run(size_t n, const Descriptors* d, int view, const uint8_t* select, const std::vector<JsonPath>& paths,
                    const Piece& piece, JsonFields& out, bool order_select = false) {
        std::vector<uint8_t> depth, names;
        std::vector<uint32_t> name_off{0};
        for (const JsonPath& p : paths) {
            if (p.names.size() > 255) throw std::invalid_argument("JsonPath: too many names");
            depth.push_back((uint8_t)p.names.size());
            for (const std::string& nm : p.names) {
                names.insert(names.end(), nm.begin(), nm.end());
                name_off.push_back((uint32_t)names.size());
            }
        }
        names.push_back(0);  // never empty
        const sbe_json_paths ps{(uint32_t)paths.size(), depth.data(), names.data(), name_off.data()};
        const size_t P = paths.size();
        out.n_paths_ = P;
        out.doc_.assign(n, SBE_JX_NOT_SELECTED);
        out.root_.assign(n, SBE_JX_MISSING);
        out.kind_.assign(n * P, SBE_JX_MISSING);
        out.off_.assign(n * P, 0);
        out.len_.assign(n * P, 0);
        sbe_json_out none{};
        if (n == 0) {  // the table and the view are still checked
            if (sbe_json_extract_batch(nullptr, nullptr, 0, nullptr, 0, nullptr, &ps, &none, nullptr, 0, nullptr) != SBE_OK ||
                (d ? (view != 3 && view != 4) : view != 0))
                throw std::invalid_argument("extract: bad path table or view");
            return;
        }
        std::vector<uint64_t> start(n + 1, 0);
        for (size_t i = 0; i < n; ++i) start[i + 1] = start[i] + piece(i).size();
        const size_t bytes = (size_t)start[n];
        const size_t o_st = al16((n + 1) * 8), o_fl = o_st + (d ? al16(n) : 0), o_vo = o_fl + (d ? al16(n) : 0),
                     o_vl = o_vo + (d ? al16(20 * n) : 0), o_hd = o_vl + (d ? al16(20 * n) : 0),
                     o_sel = o_hd + (order_select ? al16(8 * n) : 0), o_data = o_sel + (select ? al16(n) : 0),
                     stage = o_data + bytes + 16;
        // behind the staged bytes, written by the device only: the mask, pred and totals of sbe_order_select
        const size_t o_dsel = al16(stage), o_pred = o_dsel + al16(n), o_tot = o_pred + al16(n),
                     dev_bytes = order_select ? o_tot + 16 : stage;
        Ctx& c = ctx();
        Pipeline::Slot& s = c.pipe.slot[0];  // serial use of the pipeline's first slot (idle between calls)
        hipStream_t stream = c.batch_stream();
        s.pin.need(stage);
        uint8_t* hp = s.pin.b();
        std::memcpy(hp, start.data(), (n + 1) * 8);
        for_ranges(n, 4096, [&](size_t x, size_t y) {
            for (size_t i = x; i < y; ++i) {
                if (d) {
                    hp[o_st + i] = d->status(i);
                    hp[o_fl + i] = d->flags(i);
                    std::memcpy(hp + o_vo + 20 * i, d->off(i), 20);
                    std::memcpy(hp + o_vl + 20 * i, d->len(i), 20);
                    if (order_select) std::memcpy(hp + o_hd + 8 * i, d->hdr(i), 8);
                }
                if (select) hp[o_sel + i] = select[i];
                const std::string_view r = piece(i);
                if (!r.empty()) std::memcpy(hp + o_data + start[i], r.data(), r.size());
            }
        });
        s.d_in.need(dev_bytes);
        const size_t p_root = al16(n), p_kind = p_root + al16(n), p_off = p_kind + al16(n * P), p_len = p_off + al16(4 * n * P),
                     outb = p_len + al16(4 * n * P);
        s.d_out.need(outb);
        hip_check(hipMemcpyAsync(s.d_in.p, hp, stage, hipMemcpyHostToDevice, stream), "H2D");
        uint8_t* di = s.d_in.b();
        uint8_t* dq = s.d_out.b();
        const sbe_decoded dec{di + o_st, di + o_fl, order_select ? reinterpret_cast<uint16_t*>(di + o_hd) : nullptr, nullptr,
                              reinterpret_cast<uint32_t*>(di + o_vo), reinterpret_cast<uint32_t*>(di + o_vl), nullptr};
        sbe_json_out res{dq, dq + p_root, dq + p_kind, reinterpret_cast<uint32_t*>(dq + p_off),
                         reinterpret_cast<uint32_t*>(dq + p_len)};
        const uint8_t* d_select = select ? di + o_sel : nullptr;
        if (order_select) {
            const sbe_select_out so{di + o_pred, di + o_dsel, nullptr, reinterpret_cast<uint64_t*>(di + o_tot)};
            if (sbe_order_select(di + o_data, reinterpret_cast<const uint64_t*>(di), n, &dec, &so, stream) != SBE_OK) {
                c.abort_all();
                fail("sbe_order_select");
            }
            d_select = di + o_dsel;
        }
        const int rc = sbe_json_extract_batch(di + o_data, reinterpret_cast<const uint64_t*>(di), n, d ? &dec : nullptr,
                                              (uint32_t)view, d_select, &ps, &res, nullptr, 0, stream);
        if (rc == SBE_EINVAL) {
            hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
            throw std::invalid_argument("extract: bad path table or view");
        }
        if (rc != SBE_OK) {
            c.abort_all();
            fail("sbe_json_extract_batch");
        }
        auto back = [&](void* dst, size_t off, size_t len) {
            hip_check(hipMemcpyAsync(dst, dq + off, len, hipMemcpyDeviceToHost, stream), "D2H");
        };
        back(out.doc_.data(), 0, n);
        back(out.root_.data(), p_root, n);
        back(out.kind_.data(), p_kind, n * P);
        back(out.off_.data(), p_off, 4 * n * P);
        back(out.len_.data(), p_len, 4 * n * P);
        hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    }
    static std::vector<const char*>& base(JsonFields& f) { return f.base_; }
    // batch.extract(paths, 3, mask) with sbe_order_select's mask, which stays on the device
    static JsonFields order_fields(const ParsedBatch& batch, const std::vector<JsonPath>& paths) {
        JsonFields f;
        run(
            batch.n_, batch.desc_.get(), 3, nullptr, paths,
            [&](size_t i) {
                return std::string_view(reinterpret_cast<const char*>(batch.data_ + batch.rec_off_[i]),
                                        (size_t)(batch.rec_off_[i + 1] - batch.rec_off_[i]));
            },
            f, true);
        f.base_.resize(batch.n_);
        for (size_t i = 0; i < batch.n_; ++i) f.base_[i] = reinterpret_cast<const char*>(batch.data_ + batch.rec_off_[i]);
        return f;
    }
};

std::string_view JsonFields::token(std::size_t i, std::size_t p) const {
    const size_t k = i * n_paths_ + p;
    if (kind_[k] == SBE_JX_MISSING) return {};
    return {base_[i] + off_[k], len_[k]};
}

bool JsonFields::is_string(std::size_t i, std::size_t p) const {
    const uint8_t k = kind(i, p);
    return k == SBE_JX_STRING || k == SBE_JX_STRING_ESC;
}

std::string JsonFields::as_string(std::size_t i, std::size_t p) const {
    const std::string_view tok = token(i, p);
    switch (kind(i, p)) {
        case SBE_JX_STRING: return std::string(tok);
        case SBE_JX_STRING_ESC: return json_unescape(tok);
        case SBE_JX_NUMBER: return json_number_as_string(tok);
        case SBE_JX_TRUE: return "true";
        case SBE_JX_FALSE: return "false";
        case SBE_JX_OBJECT:
        case SBE_JX_ARRAY: throw std::runtime_error("Type is not convertible to string");
        default: return "";  // null, and the null Value::get gives for a missing member
    }
}

std::uint64_t JsonFields::as_uint64(std::size_t i, std::size_t p) const {
    const std::string_view t = token(i, p);
    switch (kind(i, p)) {
        case SBE_JX_MISSING:
        case SBE_JX_NULL:
        case SBE_JX_FALSE: return 0;
        case SBE_JX_TRUE: return 1;
        case SBE_JX_NUMBER: break;
        default: throw std::runtime_error("Value is not convertible to UInt64.");
    }
    // decodeNumber: an integer token that fits is an Int / UInt, everything else a real
    size_t q = 0;
    const bool neg = !t.empty() && t[0] == '-';
    if (neg) ++q;
    const uint64_t maxv = neg ? (uint64_t)1 << 63 : ~0ull, thr = maxv / 10;
    uint64_t v = 0;
    bool real = false;
    while (q < t.size() && !real) {
        const char ch = t[q++];
        if (ch < '0' || ch > '9') {
            real = true;
        } else {
            const uint64_t dg = ch - '0';
            if (v >= thr && (v > thr || q != t.size() || dg > maxv % 10)) real = true;
            else v = v * 10 + dg;
        }
    }
    if (!real) {
        if (neg && v) throw std::runtime_error("LargestInt out of UInt64 range");
        return v;
    }
    const double dv = std::strtod(std::string(t).c_str(), nullptr);
    if (!(dv >= 0.0 && dv < 18446744073709551616.0)) throw std::runtime_error("double out of UInt64 range");
    return (std::uint64_t)dv;
}

JsonFields ParsedBatch::extract(const std::vector<JsonPath>& paths, int view, const std::uint8_t* select) const {
    JsonFields f;
    if (view != 3 && view != 4) throw std::invalid_argument("extract: view is 3 (payload) or 4 (headers)");
    JsonExtractAccess::run(
        n_, desc_.get(), view, select, paths,
        [&](size_t i) {
            return std::string_view(reinterpret_cast<const char*>(data_ + rec_off_[i]), (size_t)(rec_off_[i + 1] - rec_off_[i]));
        },
        f);
    std::vector<const char*>& base = JsonExtractAccess::base(f);
    base.resize(n_);
    for (size_t i = 0; i < n_; ++i) base[i] = reinterpret_cast<const char*>(data_ + rec_off_[i]);
    return f;
}

TopicClass classify_topic(std::string_view topic) {  // include/aeron_cluster/topic_router.hpp
    if (topic == "orders" || topic == "order_request_topic") return TopicClass::Orders;
    if (topic == "_subscriptions" || topic == "_ack" || topic == "_control" || topic == "_internal")
        return TopicClass::Control;
    return TopicClass::Unknown;
}

TopicClass MessageKinds::topic_class(std::size_t i) const {
    return class_[i] == SBE_TC_ORDERS ? TopicClass::Orders : class_[i] == SBE_TC_CONTROL ? TopicClass::Control : TopicClass::Unknown;
}

MessageKinds ParsedBatch::order_select() const {
    MessageKinds k;
    const size_t n = n_;
    k.pred_.assign(n, 0);
    k.select_.assign(n, 0);
    k.class_.assign(n, SBE_TC_UNKNOWN);
    if (!n) return k;
    const Descriptors* d = desc_.get();
    const uint64_t base0 = rec_off_[0], bytes = rec_off_[n] - base0;
    // staged as extract stages a batch: rec_off rebased to 0 | status | flags | hdr | view_off |
    // view_len | the records; then, written by the device only: pred | select | class | totals
    const size_t o_st = al16((n + 1) * 8), o_fl = o_st + al16(n), o_hd = o_fl + al16(n), o_vo = o_hd + al16(8 * n),
                 o_vl = o_vo + al16(20 * n), o_data = o_vl + al16(20 * n), stage = o_data + bytes + 16;
    const size_t r_pred = 0, r_sel = al16(n), r_cls = r_sel + al16(n), r_tot = r_cls + al16(n), outb = r_tot + 16;
    Ctx& c = ctx();
    Pipeline::Slot& s = c.pipe.slot[0];  // serial use of the pipeline's first slot (idle between calls)
    hipStream_t stream = c.batch_stream();
    s.pin.need(stage);
    uint8_t* hp = s.pin.b();
    uint64_t* ro = reinterpret_cast<uint64_t*>(hp);
    for (size_t i = 0; i <= n; ++i) ro[i] = rec_off_[i] - base0;
    for_ranges(n, 4096, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) {
            hp[o_st + i] = d->status(i);
            hp[o_fl + i] = d->flags(i);
            std::memcpy(hp + o_hd + 8 * i, d->hdr(i), 8);
            std::memcpy(hp + o_vo + 20 * i, d->off(i), 20);
            std::memcpy(hp + o_vl + 20 * i, d->len(i), 20);
        }
    });
    if (bytes) std::memcpy(hp + o_data, data_ + base0, bytes);
    s.d_in.need(stage);
    s.d_out.need(outb);
    hip_check(hipMemcpyAsync(s.d_in.p, hp, stage, hipMemcpyHostToDevice, stream), "H2D");
    uint8_t* di = s.d_in.b();
    uint8_t* dq = s.d_out.b();
    const sbe_decoded dec{di + o_st, di + o_fl, reinterpret_cast<uint16_t*>(di + o_hd), nullptr,
                          reinterpret_cast<uint32_t*>(di + o_vo), reinterpret_cast<uint32_t*>(di + o_vl), nullptr};
    const sbe_select_out so{dq + r_pred, dq + r_sel, dq + r_cls, reinterpret_cast<uint64_t*>(dq + r_tot)};
    if (sbe_order_select(di + o_data, reinterpret_cast<const uint64_t*>(di), n, &dec, &so, stream) != SBE_OK) {
        c.abort_all();
        fail("sbe_order_select");
    }
    auto back = [&](void* dst, size_t off, size_t len) {
        hip_check(hipMemcpyAsync(dst, dq + off, len, hipMemcpyDeviceToHost, stream), "D2H");
    };
    back(k.pred_.data(), r_pred, n);
    back(k.select_.data(), r_sel, n);
    back(k.class_.data(), r_cls, n);
    back(k.totals_, r_tot, 16);
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    return k;
}

JsonFields extract_json_documents(const std::vector<std::string>& docs, const std::vector<JsonPath>& paths) {
    JsonFields f;
    JsonExtractAccess::run(docs.size(), nullptr, 0, nullptr, paths, [&](size_t i) { return std::string_view(docs[i]); }, f);
    std::vector<const char*>& base = JsonExtractAccess::base(f);
    base.resize(docs.size());
    for (size_t i = 0; i < docs.size(); ++i) base[i] = docs[i].data();
    return f;
}

namespace {
const std::vector<JsonPath>& order_id_paths() {
    static const std::vector<JsonPath> paths{"message",
                                             "message.message",
                                             "message.message.client_order_id",
                                             "message.message.order_id",
                                             "message.message.order_details",
                                             "message.message.order_details.client_order_id",
                                             "message.order_details",
                                             "message.order_details.client_order_id",
                                             "uuid"};
    return paths;
}
// the callback's body for one parsed document (:592-619)
OrderIds order_ids_of(const JsonFields& f, size_t i) {
    OrderIds ids;
    if (f.doc(i) != SBE_JX_OK) return ids;        // empty payload, parse failure, or the stack limit's exception
    if (f.root_kind(i) != SBE_JX_OBJECT) return ids;  // null: no member anywhere; anything else: isMember throws
    auto find_str = [&](size_t p) { return f.is_string(i, p) ? f.as_string(i, p) : std::string(); };
    const bool msg_obj = f.kind(i, 0) == SBE_JX_OBJECT;
    if (msg_obj && f.kind(i, 1) == SBE_JX_OBJECT) {  // inner.isObject()
        ids.client_order_id = find_str(2);
        ids.order_id = find_str(3);
        if (ids.client_order_id.empty() && f.kind(i, 4) == SBE_JX_OBJECT) ids.client_order_id = find_str(5);
    } else if (msg_obj && f.kind(i, 6) == SBE_JX_OBJECT) {  // the older format
        ids.client_order_id = find_str(7);
    }
    if (ids.order_id.empty()) ids.order_id = find_str(8);
    return ids;
}
bool order_callback_looks(const ParseResult& r) {  // :578-579
    return r.is_order_message() || (r.is_topic_message() && r.message_type == "CREATE_ORDER");
}
}  // namespace

std::vector<OrderIds> extract_order_ids(const ParsedBatch& batch) {
    const size_t n = batch.size();
    const JsonFields f = JsonExtractAccess::order_fields(batch, order_id_paths());  // :578-579 on the device
    std::vector<OrderIds> out(n);
    for_ranges(n, 1024, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) out[i] = order_ids_of(f, i);
    });
    return out;
}

OrderIds extract_order_ids(const ParseResult& result) {
    if (!order_callback_looks(result) || result.payload.empty()) return {};
    const std::vector<std::string> docs{result.payload};
    return order_ids_of(extract_json_documents(docs, order_id_paths()), 0);
}

// ======================================================================================
// DeliveryTracker (examples/pubsub_reconnect_test.cpp:625-716)
// ======================================================================================
namespace {
inline size_t al64(size_t v) { return (v + 63) & ~size_t(63); }

// Device layout of the three table calls' results (64-B aligned pieces).
struct TrackLayout {
    size_t mcode, mcount, ccode, ccount, scode, sval, ws, total;
    explicit TrackLayout(size_t n) {
        size_t p = 0;
        mcode = p, p = al64(p + n);
        mcount = p, p = al64(p + 4 * n);
        ccode = p, p = al64(p + n);
        ccount = p, p = al64(p + 4 * n);
        scode = p, p = al64(p + n);
        sval = p, p = al64(p + 8 * n);
        ws = p, p = al64(p + sbe_inflight_workspace_size(n));
        total = p;
    }
};

struct TrackResults {
    std::vector<uint8_t> mcode, ccode, scode;
    std::vector<uint32_t> mcount;
    std::vector<uint64_t> sval;
};
}  // namespace

struct DeliveryTracker::Impl {
    struct LongSent {
        uint64_t ts;
        bool answered;
    };
    hipStream_t stream = nullptr;
    InfTable msgs, clients, sends;
    DevBuf in, out;
    std::vector<uint8_t> stage;
    uint64_t received = 0;
    // ids the tables cannot hold
    std::unordered_map<std::string, uint64_t> long_msgs;  // message id -> deliveries
    std::unordered_set<std::string> long_clients;
    std::unordered_map<std::string, LongSent> long_sent;
    size_t long_answered = 0;
    // the recorded latencies in nanoseconds: a device log (sbe_latency_*), fed behind every lookup
    DevBuf log, log_ws, log_stage, rep;
    uint64_t log_cap = 0, log_bound = 0;  // samples it holds; an upper bound of its count
    uint64_t calls = 0;                   // on_batch / on_message calls so far: the high half of a tag
    std::vector<std::pair<size_t, uint64_t>> long_samples;  // (record, send time) of the running call's long ids

    void sync() { hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize"); }

    // room for n more samples, by reallocate-and-copy when needed
    void log_reserve(uint64_t n) {
        if (log_cap && log_bound + n <= log_cap) return;
        if (log_cap) {
            uint64_t h[3];
            hip_check(hipMemcpyAsync(h, log.p, 24, hipMemcpyDeviceToHost, stream), "D2H");
            sync();
            log_bound = h[1];
            if (log_bound + n <= log_cap) return;
        }
        uint64_t ncap = log_cap ? log_cap : 1024;
        while (log_bound + n > ncap) ncap *= 2;
        if (ncap > (1ull << 31)) throw std::runtime_error("sbecodec: the latency log cannot grow past 2^31 samples");
        DevBuf fresh;
        fresh.need(sbe_latency_log_size(ncap));
        if (sbe_latency_log_init(fresh.p, sbe_latency_log_size(ncap), ncap, stream) != SBE_OK) fail("sbe_latency_log_init");
        if (log_cap) {  // count and dropped, the latencies, the tags
            auto copy = [&](size_t to, size_t from, size_t len) {
                hip_check(hipMemcpyAsync(fresh.b() + to, log.b() + from, len, hipMemcpyDeviceToDevice, stream), "D2D");
            };
            copy(8, 8, 16);
            copy(64, 64, 8 * log_bound);
            copy(64 + 8 * ncap, 64 + 8 * log_cap, 8 * log_bound);
        }
        sync();
        std::swap(log.p, fresh.p);
        std::swap(log.cap, fresh.cap);
        log_cap = ncap;
    }

    // one sample per SBE_SENT_FIRST record of a lookup's device results
    void log_append(const uint8_t* code, const uint64_t* value, size_t n, uint64_t now_ns) {
        const size_t wsb = sbe_latency_append_workspace_size(n);
        log_ws.need(wsb);
        if (sbe_latency_append(log.p, code, value, n, now_ns, 1, calls << 32, log_ws.p, wsb, stream) != SBE_OK)
            fail("sbe_latency_append");
    }

    // the samples settle() took from long_sent, as a second append with the records' own indices
    void log_append_long(size_t n, uint64_t now_ns) {
        if (long_samples.empty()) return;
        const size_t o_code = 8 * n;
        std::vector<uint8_t> host(o_code + n, 0);  // value [n] u64 | code [n]: SBE_SENT_NONE but for the samples
        for (const auto& s : long_samples) {
            std::memcpy(host.data() + 8 * s.first, &s.second, 8);
            host[o_code + s.first] = SBE_SENT_FIRST;
        }
        log_stage.need(host.size());
        hip_check(hipMemcpyAsync(log_stage.p, host.data(), host.size(), hipMemcpyHostToDevice, stream), "H2D");
        log_append(log_stage.b() + o_code, reinterpret_cast<const uint64_t*>(log_stage.p), n, now_ns);
        sync();  // `host` goes out of scope
        long_samples.clear();
    }

    // note (message ids), note (client ids), lookup (sent) over keys that lie in a device buffer,
    // and the lookup's latencies into the log; `res` is device memory of TrackLayout(n).total bytes
    void track(const uint8_t* buf, uint64_t buf_bytes, const uint64_t* mpos, const uint32_t* mlen, const uint64_t* cpos,
               const uint32_t* clen, size_t n, uint8_t* res, TrackResults& r, uint64_t now_ns) {
        const TrackLayout L(n);
        const size_t wsb = sbe_inflight_workspace_size(n);
        msgs.reserve(n, stream);
        clients.reserve(n, stream);
        log_reserve(n);  // a record gives at most one sample, from the table or from long_sent
        log_bound += n;
        if (sbe_inflight_note_keys(msgs.p(), buf, buf_bytes, mpos, mlen, n, res + L.mcode,
                                   reinterpret_cast<uint32_t*>(res + L.mcount), nullptr, res + L.ws, wsb, stream) != SBE_OK)
            fail("sbe_inflight_note_keys");
        if (sbe_inflight_note_keys(clients.p(), buf, buf_bytes, cpos, clen, n, res + L.ccode,
                                   reinterpret_cast<uint32_t*>(res + L.ccount), nullptr, res + L.ws, wsb, stream) != SBE_OK)
            fail("sbe_inflight_note_keys");
        if (sbe_inflight_lookup_keys(sends.p(), buf, buf_bytes, cpos, clen, n, res + L.scode,
                                     reinterpret_cast<uint64_t*>(res + L.sval), nullptr, res + L.ws, wsb, stream) != SBE_OK)
            fail("sbe_inflight_lookup_keys");
        log_append(res + L.scode, reinterpret_cast<const uint64_t*>(res + L.sval), n, now_ns);
        msgs.used_bound += n;
        clients.used_bound += n;
        r.mcode.resize(n);
        r.ccode.resize(n);
        r.scode.resize(n);
        r.mcount.resize(n);
        r.sval.resize(n);
        auto back = [&](void* dst, size_t off, size_t len) {
            hip_check(hipMemcpyAsync(dst, res + off, len, hipMemcpyDeviceToHost, stream), "D2H");
        };
        back(r.mcode.data(), L.mcode, n);
        back(r.mcount.data(), L.mcount, 4 * n);
        back(r.ccode.data(), L.ccode, n);
        back(r.scode.data(), L.scode, n);
        back(r.sval.data(), L.sval, 8 * n);
        sync();
    }

    // the callback's bookkeeping for one selected record from its three codes; ids over the key
    // limit go through the host sets
    void settle(Delivery& d, std::string_view mid, const TrackResults& r, size_t i, uint64_t now_ns) {
        bool again = r.mcode[i] == SBE_DLV_AGAIN;
        d.redeliveries = again ? r.mcount[i] : 0;
        if (mid.size() > SBE_INFLIGHT_KEY_MAX) {
            uint64_t& c = long_msgs[std::string(mid)];
            again = c > 0;
            d.redeliveries = (uint32_t)c;  // on_batch writes the batch's last value afterwards
            ++c;
        }
        d.already_processed = again;
        if (!again) ++received;
        bool client_again = r.ccode[i] == SBE_DLV_AGAIN;
        if (d.client_order_id.size() > SBE_INFLIGHT_KEY_MAX) client_again = !long_clients.insert(d.client_order_id).second;
        d.duplicate_client_order = client_again && !again;
        if (d.client_order_id.size() > SBE_INFLIGHT_KEY_MAX) {
            auto it = long_sent.find(d.client_order_id);
            d.was_sent = it != long_sent.end();
            if (d.was_sent && !it->second.answered) {
                it->second.answered = true;
                ++long_answered;
                d.latency_recorded = true;
                d.latency_ns = (int64_t)now_ns - (int64_t)it->second.ts;
                long_samples.emplace_back(i, it->second.ts);
            }
        } else {
            d.was_sent = r.scode[i] == SBE_SENT_FIRST || r.scode[i] == SBE_SENT_REPEAT;
            d.latency_recorded = r.scode[i] == SBE_SENT_FIRST;
            if (d.latency_recorded) d.latency_ns = (int64_t)now_ns - (int64_t)r.sval[i];
        }
    }
};

DeliveryTracker::DeliveryTracker(std::uint64_t initial_capacity, std::uint32_t tag_bits) : impl_(new Impl) {
    Impl& m = *impl_;
    if (!sbe_inflight_table_size(initial_capacity) || tag_bits > 30)
        throw std::invalid_argument("DeliveryTracker: capacity must be a power of two in 64 .. 2^31");
    hip_check(hipStreamCreateWithFlags(&m.stream, hipStreamNonBlocking), "hipStreamCreate");
    for (InfTable* t : {&m.msgs, &m.clients, &m.sends}) t->init(initial_capacity, tag_bits, m.stream);
    m.sync();
}

DeliveryTracker::~DeliveryTracker() {
    if (impl_->stream) {
        (void)hipStreamSynchronize(impl_->stream);
        (void)hipStreamDestroy(impl_->stream);
    }
}

std::uint64_t DeliveryTracker::messages_received() const { return impl_->received; }
std::uint64_t DeliveryTracker::rehashes() const { return impl_->msgs.rehashes + impl_->clients.rehashes + impl_->sends.rehashes; }
std::size_t DeliveryTracker::sent() const {
    uint64_t h[5];
    impl_->sends.header(h, impl_->stream);
    return (size_t)h[1] + impl_->long_sent.size();
}
std::size_t DeliveryTracker::received() const {
    uint64_t h[5];
    impl_->clients.header(h, impl_->stream);
    return (size_t)h[1] + impl_->long_clients.size();
}
std::size_t DeliveryTracker::missing() const {
    uint64_t h[5];
    impl_->sends.header(h, impl_->stream);
    return (size_t)(h[1] - h[4]) + impl_->long_sent.size() - impl_->long_answered;
}
std::size_t DeliveryTracker::extra() const {
    uint64_t h[5];
    impl_->sends.header(h, impl_->stream);
    return received() - (size_t)h[4] - impl_->long_answered;
}

void DeliveryTracker::clear_duplicate_tracking() {
    Impl& m = *impl_;
    if (sbe_inflight_reset_values(m.msgs.p(), m.stream) != SBE_OK) fail("sbe_inflight_reset_values");
    m.sync();
    for (auto& kv : m.long_msgs) kv.second = 1;
}

namespace {
// The first `limit` entries of `table` that pass (sbe_inflight_list_keys) merged with `host`, the
// passing ids the tables cannot hold: both in std::string order, so the merge looks at no more
// than limit + host.size() entries.
IdList list_ids(const InfTable& table, const InfTable* other, uint64_t min_value, size_t limit, std::vector<IdEntry> host,
                DevBuf& dev, hipStream_t stream) {
    if (limit > SBE_LIST_MAX) throw std::invalid_argument("DeliveryTracker: a list holds at most SBE_LIST_MAX ids");
    const uint32_t k = (uint32_t)limit;
    const size_t o_key = 64, o_len = o_key + al64(SBE_INFLIGHT_KEY_MAX * SBE_LIST_MAX), o_val = o_len + 4 * SBE_LIST_MAX,
                 o_ans = o_val + 8 * SBE_LIST_MAX, o_ws = o_ans + SBE_LIST_MAX, wsb = sbe_inflight_list_workspace_size(k);
    dev.need(o_ws + wsb);
    uint8_t* d = dev.b();
    const sbe_key_list_out out{reinterpret_cast<uint64_t*>(d), d + o_key, reinterpret_cast<uint32_t*>(d + o_len),
                               reinterpret_cast<uint64_t*>(d + o_val), d + o_ans};
    if (sbe_inflight_list_keys(table.p(), other ? other->p() : nullptr, other ? SBE_LIST_NOT_IN_OTHER : 0, min_value, k, &out,
                               d + o_ws, wsb, stream) != SBE_OK)
        fail("sbe_inflight_list_keys");
    std::vector<uint8_t> back(o_ans);
    hip_check(hipMemcpyAsync(back.data(), d, o_ans, hipMemcpyDeviceToHost, stream), "D2H");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    uint64_t count;
    std::memcpy(&count, back.data(), 8);
    const size_t rows = (size_t)std::min<uint64_t>(count, k);
    std::vector<IdEntry> listed(rows);
    for (size_t j = 0; j < rows; ++j) {
        uint32_t len;
        std::memcpy(&len, back.data() + o_len + 4 * j, 4);
        listed[j].id.assign(reinterpret_cast<const char*>(back.data() + o_key + SBE_INFLIGHT_KEY_MAX * j), len);
        std::memcpy(&listed[j].value, back.data() + o_val + 8 * j, 8);
    }
    std::sort(host.begin(), host.end(), [](const IdEntry& a, const IdEntry& b) { return a.id < b.id; });
    IdList res;
    res.total = (size_t)count + host.size();
    res.first.resize(listed.size() + host.size());
    std::merge(listed.begin(), listed.end(), host.begin(), host.end(), res.first.begin(),
               [](const IdEntry& a, const IdEntry& b) { return a.id < b.id; });
    if (res.first.size() > limit) res.first.resize(limit);
    return res;
}
}  // namespace

IdList DeliveryTracker::missing_ids(std::size_t limit) const {
    Impl& m = *impl_;
    std::vector<IdEntry> host;
    for (const auto& kv : m.long_sent)
        if (!m.long_clients.count(kv.first)) host.push_back({kv.first, kv.second.ts});
    return list_ids(m.sends, &m.clients, 0, limit, std::move(host), m.rep, m.stream);
}

IdList DeliveryTracker::extra_ids(std::size_t limit) const {
    Impl& m = *impl_;
    std::vector<IdEntry> host;
    for (const std::string& id : m.long_clients)
        if (!m.long_sent.count(id)) host.push_back({id, 0});
    return list_ids(m.clients, &m.sends, 0, limit, std::move(host), m.rep, m.stream);
}

IdList DeliveryTracker::redelivered_ids(std::size_t limit) const {
    Impl& m = *impl_;
    std::vector<IdEntry> host;
    for (const auto& kv : m.long_msgs)
        if (kv.second >= 2) host.push_back({kv.first, kv.second});
    IdList res = list_ids(m.msgs, nullptr, 2, limit, std::move(host), m.rep, m.stream);
    for (IdEntry& e : res.first) --e.value;  // deliveries -> redeliveries
    return res;
}

LatencyReport DeliveryTracker::latency_report(const std::vector<double>& pcts, std::uint64_t unit_ns, bool want_rows) const {
    Impl& m = *impl_;
    if (pcts.size() > SBE_LAT_MAX_PCT || unit_ns < 1 || unit_ns > (1ull << 62))
        throw std::invalid_argument("DeliveryTracker::latency_report: at most 16 percentiles, unit_ns in 1 .. 2^62");
    for (double p : pcts)
        if (!(p >= 0.0 && p <= 100.0)) throw std::invalid_argument("DeliveryTracker::latency_report: a percentile outside [0, 100]");
    LatencyReport res;
    res.percentiles.assign(pcts.size(), 0);
    if (!m.log_cap) return res;  // nothing was ever tracked
    const bool rows = want_rows || unit_ns != 1;  // the sorted samples are needed on the host
    const size_t np = SBE_LAT_MAX_PCT, o_stats = 64, o_pv = 128, o_pi = o_pv + 8 * np, o_sorted = o_pi + 8 * np,
                 o_order = o_sorted + (rows ? al64(8 * m.log_cap) : 0), o_ws = o_order + (rows ? al64(4 * m.log_cap) : 0),
                 wsb = sbe_latency_report_workspace_size(m.log_cap);
    m.rep.need(o_ws + wsb);
    uint8_t* d = m.rep.b();
    const sbe_latency_report_out out{reinterpret_cast<uint64_t*>(d), reinterpret_cast<int64_t*>(d + o_stats),
                                     reinterpret_cast<int64_t*>(d + o_pv), reinterpret_cast<uint64_t*>(d + o_pi),
                                     rows ? reinterpret_cast<int64_t*>(d + o_sorted) : nullptr,
                                     rows ? reinterpret_cast<uint32_t*>(d + o_order) : nullptr};
    if (sbe_latency_report(m.log.p, pcts.data(), (uint32_t)pcts.size(), &out, d + o_ws, wsb, m.stream) != SBE_OK)
        fail("sbe_latency_report");
    std::vector<uint8_t> head(o_sorted);
    hip_check(hipMemcpyAsync(head.data(), d, o_sorted, hipMemcpyDeviceToHost, m.stream), "D2H");
    m.sync();
    int64_t stats[3];
    std::memcpy(&res.count, head.data(), 8);
    std::memcpy(stats, head.data() + o_stats, 24);
    const int64_t unit = (int64_t)unit_ns;
    res.sum = stats[0];
    res.min = stats[1] / unit;
    res.max = stats[2] / unit;
    for (size_t p = 0; p < pcts.size(); ++p) {
        int64_t v;
        std::memcpy(&v, head.data() + o_pv + 8 * p, 8);
        res.percentiles[p] = v / unit;
    }
    if (rows && res.count) {
        const size_t n = (size_t)res.count;
        std::vector<int64_t> sorted(n);
        hip_check(hipMemcpyAsync(sorted.data(), d + o_sorted, 8 * n, hipMemcpyDeviceToHost, m.stream), "D2H");
        std::vector<uint32_t> order;
        std::vector<uint64_t> tags;
        if (want_rows) {
            order.resize(n);
            tags.resize(n);  // positions below the count
            hip_check(hipMemcpyAsync(order.data(), d + o_order, 4 * n, hipMemcpyDeviceToHost, m.stream), "D2H");
            hip_check(hipMemcpyAsync(tags.data(), m.log.b() + 64 + 8 * m.log_cap, 8 * n, hipMemcpyDeviceToHost, m.stream), "D2H");
        }
        m.sync();
        if (unit_ns != 1) {  // the sum of the divided samples, mod 2^64
            uint64_t s = 0;
            for (int64_t v : sorted) s += (uint64_t)(v / unit);
            res.sum = (int64_t)s;
        }
        if (want_rows) {
            res.rows.resize(n);
            for (size_t j = 0; j < n; ++j) res.rows[j] = LatencyRow{sorted[n - 1 - j] / unit, tags[order[n - 1 - j]]};
        }
    }
    res.avg = res.count ? (double)res.sum / (double)res.count : 0.0;
    return res;
}

void DeliveryTracker::note_sent(const std::vector<std::string>& ids, std::uint64_t ts_ns) {
    Impl& m = *impl_;
    // staged: key_off [k] u32, key_len [k] u32, key bytes
    size_t k = 0, bytes = 0;
    for (const std::string& u : ids) {
        if (u.size() <= SBE_INFLIGHT_KEY_MAX) {
            ++k;
            bytes += u.size();
        } else {
            m.long_sent.emplace(u, Impl::LongSent{ts_ns, false});
        }
    }
    if (!k) return;
    if (bytes > 0xffffffffull) throw std::invalid_argument("DeliveryTracker::note_sent: more than 4 GiB of ids");
    const size_t o_len = 4 * k, o_key = 8 * k, total = o_key + bytes + 16;
    m.stage.resize(total);
    uint32_t* off = reinterpret_cast<uint32_t*>(m.stage.data());
    uint32_t* len = reinterpret_cast<uint32_t*>(m.stage.data() + o_len);
    size_t j = 0, pos = 0;
    for (const std::string& u : ids) {
        if (u.size() > SBE_INFLIGHT_KEY_MAX) continue;
        off[j] = (uint32_t)pos;
        len[j] = (uint32_t)u.size();
        std::memcpy(m.stage.data() + o_key + pos, u.data(), u.size());
        pos += u.size();
        ++j;
    }
    m.sends.reserve(k, m.stream);
    const size_t wsb = sbe_inflight_workspace_size(k);
    m.in.need(total);
    m.out.need(wsb);
    hip_check(hipMemcpyAsync(m.in.p, m.stage.data(), total, hipMemcpyHostToDevice, m.stream), "H2D");
    if (sbe_inflight_remember(m.sends.p(), m.in.b() + o_key, reinterpret_cast<const uint32_t*>(m.in.p),
                              reinterpret_cast<const uint32_t*>(m.in.b() + o_len), 1, nullptr, ts_ns, nullptr, k, nullptr,
                              m.out.p, wsb, m.stream) != SBE_OK)
        fail("sbe_inflight_remember");
    m.sync();  // the staging buffer is reused by the next call
    m.sends.used_bound += k;
}

Delivery DeliveryTracker::on_message(const ParseResult& result, std::uint64_t now_ns) {
    Impl& m = *impl_;
    Delivery d;
    d.selected = order_callback_looks(result);
    if (!d.selected) return d;
    OrderIds ids = extract_order_ids(result);
    d.client_order_id = std::move(ids.client_order_id);
    d.order_id = std::move(ids.order_id);
    // a one-record batch of keys: the two ids back to back; ids the tables cannot hold get no key
    const std::string& mid = result.message_id;
    const std::string& cid = d.client_order_id;
    const size_t o_cpos = 8, o_mlen = 16, o_clen = 20, o_key = 64, total = o_key + mid.size() + cid.size() + 16;
    m.stage.assign(total, 0);
    const uint64_t mpos = 0, cpos = mid.size();
    const uint32_t mlen = mid.empty() || mid.size() > SBE_INFLIGHT_KEY_MAX ? SBE_NO_KEY : (uint32_t)mid.size();
    const uint32_t clen = cid.empty() || cid.size() > SBE_INFLIGHT_KEY_MAX ? SBE_NO_KEY : (uint32_t)cid.size();
    std::memcpy(m.stage.data(), &mpos, 8);
    std::memcpy(m.stage.data() + o_cpos, &cpos, 8);
    std::memcpy(m.stage.data() + o_mlen, &mlen, 4);
    std::memcpy(m.stage.data() + o_clen, &clen, 4);
    std::memcpy(m.stage.data() + o_key, mid.data(), mid.size());
    std::memcpy(m.stage.data() + o_key + mid.size(), cid.data(), cid.size());
    m.in.need(total);
    m.out.need(TrackLayout(1).total);
    hip_check(hipMemcpyAsync(m.in.p, m.stage.data(), total, hipMemcpyHostToDevice, m.stream), "H2D");
    TrackResults r;
    m.track(m.in.b() + o_key, mid.size() + cid.size(), reinterpret_cast<const uint64_t*>(m.in.p),
            reinterpret_cast<const uint32_t*>(m.in.b() + o_mlen), reinterpret_cast<const uint64_t*>(m.in.b() + o_cpos),
            reinterpret_cast<const uint32_t*>(m.in.b() + o_clen), 1, m.out.b(), r, now_ns);
    m.settle(d, mid, r, 0, now_ns);
    m.log_append_long(1, now_ns);
    ++m.calls;
    return d;
}

std::vector<Delivery> DeliveryTracker::on_batch(const ParsedBatch& batch, std::uint64_t now_ns) {
    Impl& m = *impl_;
    const size_t n = batch.size();
    std::vector<Delivery> res(n);
    if (!n) return res;
    const Descriptors* d = batch.desc_.get();
    const uint64_t base0 = batch.rec_off_[0], bytes = batch.rec_off_[n] - base0;
    const char* host = reinterpret_cast<const char*>(batch.data_ + base0);
    constexpr size_t P = SBE_DLV_PATHS;
    // staged: rec_off rebased to 0 [n + 1] | status | flags | view_off | view_len | hdr | the
    // records | room for the decoded forms of escaped ids (never longer than their tokens)
    const size_t o_st = al64(8 * (n + 1)), o_fl = o_st + al64(n), o_vo = o_fl + al64(n), o_vl = o_vo + al64(20 * n),
                 o_hd = o_vl + al64(20 * n), o_data = o_hd + al64(8 * n), total_in = o_data + 2 * bytes + 16;
    m.stage.resize(o_data + bytes);
    uint8_t* hp = m.stage.data();
    uint64_t* ro = reinterpret_cast<uint64_t*>(hp);
    for (size_t i = 0; i <= n; ++i) ro[i] = batch.rec_off_[i] - base0;
    for_ranges(n, 4096, [&](size_t x, size_t y) {
        for (size_t i = x; i < y; ++i) {
            hp[o_st + i] = d->status(i);
            hp[o_fl + i] = d->flags(i);
            std::memcpy(hp + o_vo + 20 * i, d->off(i), 20);
            std::memcpy(hp + o_vl + 20 * i, d->len(i), 20);
            std::memcpy(hp + o_hd + 8 * i, d->hdr(i), 8);
        }
    });
    if (bytes) std::memcpy(hp + o_data, host, bytes);
    // results: the extract's five arrays | the keys' nine and totals | the table calls' results
    const TrackLayout L(n);
    size_t q = 0;
    const size_t j_doc = q; q = al64(q + n);
    const size_t j_root = q; q = al64(q + n);
    const size_t j_kind = q; q = al64(q + P * n);
    const size_t j_off = q; q = al64(q + 4 * P * n);
    const size_t j_len = q; q = al64(q + 4 * P * n);
    const size_t k_mpos = q; q = al64(q + 8 * n);
    const size_t k_mlen = q; q = al64(q + 4 * n);
    const size_t k_cpos = q; q = al64(q + 8 * n);
    const size_t k_clen = q; q = al64(q + 4 * n);
    const size_t k_ckind = q; q = al64(q + n);
    const size_t k_opos = q; q = al64(q + 8 * n);
    const size_t k_olen = q; q = al64(q + 4 * n);
    const size_t k_okind = q; q = al64(q + n);
    const size_t k_sel = q; q = al64(q + n);
    const size_t k_tot = q; q = al64(q + 16);
    const size_t s_sel = q; q = al64(q + n);  // sbe_order_select: the callback's outer if (:578-579), pred, totals
    const size_t s_pred = q; q = al64(q + n);
    const size_t s_tot = q; q = al64(q + 16);
    const size_t o_res = q;
    m.in.need(total_in);
    m.out.need(o_res + L.total);
    hip_check(hipMemcpyAsync(m.in.p, hp, o_data + bytes, hipMemcpyHostToDevice, m.stream), "H2D");
    uint8_t* di = m.in.b();
    uint8_t* dq = m.out.b();
    const uint64_t* d_ro = reinterpret_cast<const uint64_t*>(di);
    const sbe_decoded dec{di + o_st, di + o_fl, reinterpret_cast<uint16_t*>(di + o_hd), nullptr,
                          reinterpret_cast<uint32_t*>(di + o_vo), reinterpret_cast<uint32_t*>(di + o_vl), nullptr};
    {
        const sbe_select_out so{dq + s_pred, dq + s_sel, nullptr, reinterpret_cast<uint64_t*>(dq + s_tot)};
        if (sbe_order_select(di + o_data, d_ro, n, &dec, &so, m.stream) != SBE_OK) fail("sbe_order_select");
        std::vector<uint8_t> depth, names;
        std::vector<uint32_t> name_off{0};
        for (const JsonPath& p : order_id_paths()) {
            depth.push_back((uint8_t)p.names.size());
            for (const std::string& nm : p.names) {
                names.insert(names.end(), nm.begin(), nm.end());
                name_off.push_back((uint32_t)names.size());
            }
        }
        const sbe_json_paths ps{(uint32_t)depth.size(), depth.data(), names.data(), name_off.data()};
        sbe_json_out jo{dq + j_doc, dq + j_root, dq + j_kind, reinterpret_cast<uint32_t*>(dq + j_off),
                        reinterpret_cast<uint32_t*>(dq + j_len)};
        if (sbe_json_extract_batch(di + o_data, d_ro, n, &dec, 3, dq + s_sel, &ps, &jo, nullptr, 0, m.stream) != SBE_OK)
            fail("sbe_json_extract_batch");
        const sbe_delivery_key_out ko{reinterpret_cast<uint64_t*>(dq + k_mpos), reinterpret_cast<uint32_t*>(dq + k_mlen),
                                      reinterpret_cast<uint64_t*>(dq + k_cpos), reinterpret_cast<uint32_t*>(dq + k_clen),
                                      dq + k_ckind,
                                      reinterpret_cast<uint64_t*>(dq + k_opos), reinterpret_cast<uint32_t*>(dq + k_olen),
                                      dq + k_okind, dq + k_sel, reinterpret_cast<uint64_t*>(dq + k_tot)};
        if (sbe_delivery_keys(d_ro, n, &dec, dq + s_sel, &jo, &ko, m.stream) != SBE_OK) fail("sbe_delivery_keys");
    }
    std::vector<uint64_t> mpos(n), cpos(n), opos(n);
    std::vector<uint32_t> mlen(n), clen(n), olen(n);
    std::vector<uint8_t> ckind(n), okind(n), sel(n);
    uint64_t totals[2] = {0, 0};
    auto back = [&](void* dst, size_t off, size_t len) {
        hip_check(hipMemcpyAsync(dst, dq + off, len, hipMemcpyDeviceToHost, m.stream), "D2H");
    };
    back(mpos.data(), k_mpos, 8 * n);
    back(mlen.data(), k_mlen, 4 * n);
    back(cpos.data(), k_cpos, 8 * n);
    back(clen.data(), k_clen, 4 * n);
    back(ckind.data(), k_ckind, n);
    back(opos.data(), k_opos, 8 * n);
    back(olen.data(), k_olen, 4 * n);
    back(okind.data(), k_okind, n);
    back(sel.data(), k_sel, n);
    back(totals, k_tot, 16);
    m.sync();
    // the id strings, cut from the caller's bytes; escaped ones decoded, and the decoded client ids
    // appended behind the staged batch so that the tables compare what decodeString gives
    std::vector<uint8_t> extra;
    bool patched = false;
    for (size_t i = 0; i < n; ++i) {
        if (!sel[i]) continue;
        Delivery& r = res[i];
        r.selected = true;
        if (clen[i] != SBE_NO_KEY) {
            const std::string_view tok(host + cpos[i], clen[i]);
            if (ckind[i] == SBE_JX_STRING_ESC) {
                r.client_order_id = json_unescape(tok);
                cpos[i] = bytes + extra.size();
                clen[i] = (uint32_t)r.client_order_id.size();
                extra.insert(extra.end(), r.client_order_id.begin(), r.client_order_id.end());
                patched = true;
            } else {
                r.client_order_id.assign(tok);
            }
        }
        if (olen[i] != SBE_NO_KEY) {
            const std::string_view tok(host + opos[i], olen[i]);
            r.order_id = okind[i] == SBE_JX_STRING_ESC ? json_unescape(tok) : std::string(tok);
        }
    }
    if (patched) {
        if (!extra.empty())
            hip_check(hipMemcpyAsync(di + o_data + bytes, extra.data(), extra.size(), hipMemcpyHostToDevice, m.stream), "H2D");
        hip_check(hipMemcpyAsync(dq + k_cpos, cpos.data(), 8 * n, hipMemcpyHostToDevice, m.stream), "H2D");
        hip_check(hipMemcpyAsync(dq + k_clen, clen.data(), 4 * n, hipMemcpyHostToDevice, m.stream), "H2D");
    }
    TrackResults tr;
    m.track(di + o_data, bytes + extra.size(), reinterpret_cast<const uint64_t*>(dq + k_mpos),
            reinterpret_cast<const uint32_t*>(dq + k_mlen), reinterpret_cast<const uint64_t*>(dq + k_cpos),
            reinterpret_cast<const uint32_t*>(dq + k_clen), n, dq + o_res, tr, now_ns);
    bool long_ids = false;
    for (size_t i = 0; i < n; ++i) {
        if (!sel[i]) continue;
        const std::string_view mid = mlen[i] == SBE_NO_KEY ? std::string_view() : std::string_view(host + mpos[i], mlen[i]);
        m.settle(res[i], mid, tr, i, now_ns);
        long_ids |= mid.size() > SBE_INFLIGHT_KEY_MAX;
    }
    m.log_append_long(n, now_ns);
    ++m.calls;
    if (long_ids)  // as for the table's ids: the count recorded after the whole batch
        for (size_t i = 0; i < n; ++i)
            if (sel[i] && mlen[i] != SBE_NO_KEY && mlen[i] > SBE_INFLIGHT_KEY_MAX && res[i].already_processed)
                res[i].redeliveries = (uint32_t)(m.long_msgs[std::string(host + mpos[i], mlen[i])] - 1);
    return res;
}

std::vector<CommitOffset> CommitManager::parse_commit_offsets_batch(const std::vector<std::string>& payloads,
                                                                    std::vector<std::string>* errors) {
    static const std::vector<JsonPath> paths{"topic", "message_identifier", "message_id", "timestamp_nanos",
                                             "sequence_number"};
    const JsonFields f = extract_json_documents(payloads, paths);
    std::vector<CommitOffset> out(payloads.size());
    if (errors) errors->assign(payloads.size(), "");
    for (size_t i = 0; i < payloads.size(); ++i) {
        try {
            if (f.doc(i) == SBE_JX_STACK) throw std::runtime_error("Exceeded stackLimit in readValue().");  // the reader's own
            if (f.doc(i) != SBE_JX_OK) throw std::runtime_error("Failed to parse commit offset JSON: document does not parse");
            if (f.root_kind(i) != SBE_JX_OBJECT && f.root_kind(i) != SBE_JX_NULL)  // Value::get
                throw std::runtime_error("in Json::Value::find(begin, end): requires objectValue or nullValue");
            CommitOffset o;
            o.topic = f.as_string(i, 0);
            o.message_identifier = f.as_string(i, 1);
            o.message_id = f.as_string(i, 2);
            o.timestamp_nanos = f.as_uint64(i, 3);
            o.sequence_number = f.as_uint64(i, 4);
            out[i] = std::move(o);
        } catch (const std::runtime_error& e) {
            if (!errors) throw;
            (*errors)[i] = e.what();
        }
    }
    return out;
}

CommitOffset CommitManager::parse_commit_offset(const std::string& payload) {
    return parse_commit_offsets_batch(std::vector<std::string>{payload}).front();
}

}  // namespace aeron_cluster
