// spl_host_res.h -- what the host side of the library OWNS: the error helper and HIP_TRY, one owner per kind of GPU resource (device
// allocation, mapped pinned block, event, stream), the pinned-buffer pool and the HSA/SDMA binding, the trace macros.  Needs nothing of
// the library but SPL_* codes (include/splintr_hip.h); every other host file builds on it.
#pragma once
namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(SPL_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)
#define SPL_TRY(expr)                                                                      \
    do {                                                                                   \
        const int rc_ = (expr);                                                            \
        if (rc_ != SPL_OK) return rc_;                                                     \
    } while (0)

// One hipMalloc allocation of T's.  Move-only (the move operations delete the copies); freed by the destructor.  The kernels take the plain pointer (get()).
template <class T> struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    // n fresh elements (uninitialised) in place of what it held; the caller has made sure nothing on the device still uses that
    int alloc(size_t n) {
        reset();
        HIP_TRY(hipMalloc((void**)&p_, n ? n * sizeof(T) : 16));
        return SPL_OK;
    }
    int alloc_zeroed(size_t n) {
        SPL_TRY(alloc(n));
        HIP_TRY(hipMemset(p_, 0, n * sizeof(T)));
        return SPL_OK;
    }
    int upload(const std::vector<T>& v) {
        SPL_TRY(alloc(v.size()));
        if (!v.empty()) HIP_TRY(hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return SPL_OK;
    }
    // Grow-only scratch: holds `need` elements already (*cap) -> nothing; else wait until the device -- or, given a stream, only that
    // stream -- is through with the old allocation, free it and allocate new_cap elements.  The caller names new_cap: its formula sets
    // how often a steady workload allocates again.
    int grow(uint64_t* cap, uint64_t need, uint64_t new_cap, const hipStream_t* only_stream = nullptr) {
        if (need <= *cap && p_) return SPL_OK;
        if (only_stream) HIP_TRY(hipStreamSynchronize(*only_stream));
        else HIP_TRY(hipDeviceSynchronize());
        *cap = 0;
        SPL_TRY(alloc(new_cap));
        *cap = new_cap;
        return SPL_OK;
    }
private:
    T* p_ = nullptr;
};

// One block of mapped pinned host memory (zero-filled) and the address the device sees it at.  Move-only, as DevBuf.
template <class T> struct HostMapped {
    HostMapped() = default;
    HostMapped(HostMapped&& o) noexcept : h_(o.h_), d_(o.d_) { o.h_ = nullptr; o.d_ = nullptr; }
    HostMapped& operator=(HostMapped&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; d_ = o.d_; o.h_ = nullptr; o.d_ = nullptr; } return *this; }
    ~HostMapped() { reset(); }
    T* host() const { return h_; }
    T* dev() const { return d_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset() { if (h_) (void)hipHostFree(h_); h_ = nullptr; d_ = nullptr; }
    int alloc(size_t n, unsigned flags = hipHostMallocPortable) {
        reset();
        HIP_TRY(hipHostMalloc((void**)&h_, n * sizeof(T), flags));
        memset(h_, 0, n * sizeof(T));
        void* dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, h_, 0));
        d_ = (T*)dp;
        return SPL_OK;
    }
private:
    T* h_ = nullptr;
    T* d_ = nullptr;
};

// hipEvent_t / hipStream_t: null until created, destroyed if set.  Move-only.
template <class H, hipError_t (*Destroy)(H)> struct Owned {
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
    ~Owned() { reset(); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset(H take = nullptr) { if (h_) (void)Destroy(h_); h_ = take; }      // (take: a stream the probe picked, owned from here on)
protected:
    H h_ = nullptr;
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    int create(unsigned flags = hipEventDisableTiming) { reset(); HIP_TRY(hipEventCreateWithFlags(&h_, flags)); return SPL_OK; }
};
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    int create() { reset(); HIP_TRY(hipStreamCreateWithFlags(&h_, hipStreamNonBlocking)); return SPL_OK; }
};

// Pinned host buffers are expensive to create (the driver pins and maps every page), so result and
// staging buffers are recycled.  Shared by the handle and by the results it gave out: a result
// may outlive its handle.
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<size_t, void*>> free_;
    size_t held = 0;
    static constexpr size_t HELD_MAX = 8ull << 30;
    void* get(size_t need, size_t& cap) {
        need = std::max<size_t>(need, 4096);
        {
            std::lock_guard<std::mutex> g(mu);
            int best = -1;
            // (no buffer is smaller than 64 KiB: a request below that must still find the one it returned last
            //  time -- it did not, and every call with a small offsets array paid a hipHostMalloc, 20 us)
            const size_t lim = 4 * std::max<size_t>(need, (size_t)1 << 16);
            for (int i = 0; i < (int)free_.size(); i++)
                if (free_[i].first >= need && free_[i].first <= lim && (best < 0 || free_[i].first < free_[best].first)) best = i;
            if (best >= 0) {
                void* p = free_[best].second;
                cap = free_[best].first;
                held -= cap;
                free_.erase(free_.begin() + best);
                return p;
            }
        }
        size_t c = 1 << 16;
        while (c < need) c <<= 1;
        if (c > (64u << 20)) c = (need + (32u << 20) - 1) / (32u << 20) * (32u << 20);     // big ones: 32 MiB steps
        void* p = nullptr;
        if (hipHostMalloc(&p, c, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        cap = c;
        return p;
    }
    void put(void* p, size_t cap) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> g(mu);
            if (held + cap <= HELD_MAX) { free_.emplace_back(cap, p); held += cap; return; }
        }
        (void)hipHostFree(p);
    }
    ~PinnedPool() { for (auto& f : free_) (void)hipHostFree(f.second); }
};

// One pinned buffer from the pool, returned on scope exit.
struct Pinned {
    std::shared_ptr<PinnedPool> pool;
    void* p = nullptr;
    size_t cap = 0;
    bool ensure(const std::shared_ptr<PinnedPool>& pl, size_t need) {
        if (p && cap >= need) return true;
        release();
        pool = pl;
        p = pool->get(need, cap);
        return p != nullptr;
    }
    void release() { if (p && pool) pool->put(p, cap); p = nullptr; cap = 0; }
    ~Pinned() { release(); }
};

// Pinned buffers handed to the caller as plain pointers (spl_decode_batch's outputs): spl_free finds the pool
// they go back to here; a pointer it does not know is malloc'd memory.
struct LooseBuffers {
    std::mutex mu;
    std::unordered_map<void*, std::pair<std::shared_ptr<PinnedPool>, size_t>> m;
    void add(void* p, const std::shared_ptr<PinnedPool>& pool, size_t cap) { std::lock_guard<std::mutex> g(mu); m[p] = {pool, cap}; }
    bool release(void* p) {
        std::pair<std::shared_ptr<PinnedPool>, size_t> e;
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = m.find(p);
            if (it == m.end()) return false;
            e = it->second;
            m.erase(it);
        }
        e.first->put(p, e.second);
        return true;
    }
};
LooseBuffers& loose() { static LooseBuffers* l = new LooseBuffers(); return *l; }   // (never destroyed: results may outlive every handle)

// The DMA engines driven directly (VERDICT r04 #5a): hipMemcpyAsync device -> pinned host runs as a SHADER copy on this stack
// (__amd_rocclr_copyBuffer: 7 % of the GPU time of the C3 pipeline, and it slows the next chunk's tile kernel while it runs);
// hsa_amd_memory_async_copy hands the same copy to an SDMA engine.  libhsa-runtime64 is the runtime HIP itself sits on (already in
// the process); its entry points are bound with dlsym so that the library gains no link dependency.  Option "sdma_d2h".
struct HsaDma {
    bool ok = false;
    std::string err;
    hsa_agent_t cpu{};
    std::vector<hsa_agent_t> gpus;
    decltype(&hsa_init) Init = nullptr;
    decltype(&hsa_iterate_agents) IterateAgents = nullptr;
    decltype(&hsa_agent_get_info) AgentGetInfo = nullptr;
    decltype(&hsa_signal_create) SignalCreate = nullptr;
    decltype(&hsa_signal_destroy) SignalDestroy = nullptr;
    decltype(&hsa_signal_store_relaxed) SignalStore = nullptr;
    decltype(&hsa_signal_wait_scacquire) SignalWait = nullptr;
    decltype(&hsa_amd_memory_async_copy) AsyncCopy = nullptr;
    static hsa_status_t on_agent(hsa_agent_t a, void* self) {
        HsaDma* h = (HsaDma*)self;
        hsa_device_type_t ty;
        if (h->AgentGetInfo(a, HSA_AGENT_INFO_DEVICE, &ty) != HSA_STATUS_SUCCESS) return HSA_STATUS_SUCCESS;
        if (ty == HSA_DEVICE_TYPE_GPU) h->gpus.push_back(a);
        else if (ty == HSA_DEVICE_TYPE_CPU && h->cpu.handle == 0) h->cpu = a;
        return HSA_STATUS_SUCCESS;
    }
    void load() {
        void* lib = dlopen("libhsa-runtime64.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { const char* e = dlerror(); err = std::string("libhsa-runtime64 not found: ") + (e ? e : ""); return; }
        auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p && err.empty()) err = std::string("libhsa-runtime64 lacks ") + n; return p; };
        Init = (decltype(Init))sym("hsa_init");
        IterateAgents = (decltype(IterateAgents))sym("hsa_iterate_agents");
        AgentGetInfo = (decltype(AgentGetInfo))sym("hsa_agent_get_info");
        SignalCreate = (decltype(SignalCreate))sym("hsa_signal_create");
        SignalDestroy = (decltype(SignalDestroy))sym("hsa_signal_destroy");
        SignalStore = (decltype(SignalStore))sym("hsa_signal_store_relaxed");
        SignalWait = (decltype(SignalWait))sym("hsa_signal_wait_scacquire");
        AsyncCopy = (decltype(AsyncCopy))sym("hsa_amd_memory_async_copy");
        if (!err.empty()) return;
        if (Init() != HSA_STATUS_SUCCESS) { err = "hsa_init failed"; return; }          // (reference counted: HIP has initialised it already)
        if (IterateAgents(&HsaDma::on_agent, this) != HSA_STATUS_SUCCESS || gpus.empty() || cpu.handle == 0) { err = "no HSA agents"; return; }
        ok = true;
    }
};
HsaDma& hsa_dma() { static HsaDma* h = [] { auto* p = new HsaDma(); p->load(); return p; }(); return *h; }
// the HSA agent of a HIP device: matched by PCI bus / device / function (HIP_VISIBLE_DEVICES may reorder or hide devices); false if none
bool hsa_agent_of(int hip_device, hsa_agent_t* out) {
    HsaDma& H = hsa_dma();
    if (!H.ok) return false;
    int bus = -1, dev = -1, dom = 0;
    if (hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, hip_device) != hipSuccess ||
        hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, hip_device) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, hip_device) != hipSuccess) { (void)hipGetLastError(); dom = 0; }
    for (hsa_agent_t a : H.gpus) {
        uint32_t bdf = 0, adom = 0;
        if (H.AgentGetInfo(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_BDFID, &bdf) != HSA_STATUS_SUCCESS) continue;
        (void)H.AgentGetInfo(a, (hsa_agent_info_t)HSA_AMD_AGENT_INFO_DOMAIN, &adom);
        if ((int)((bdf >> 8) & 0xFFu) == bus && (int)((bdf >> 3) & 0x1Fu) == dev && (int)adom == dom) { *out = a; return true; }
    }
    return false;
}

// SPL_TRACE=1: progress of the host pipeline on stderr (development aid)
bool trace_on() { static const bool on = getenv("SPL_TRACE") != nullptr; return on; }
#ifdef SPL_HOST_TIMING   /* dev build: average host time between marks of the one-chunk path, printed every 256 calls */
#include <chrono>
static double g_ht[8]; static int g_htn;
#define HT_T(v) const auto v = std::chrono::steady_clock::now()
#define HT_ACC(i, a, b_) g_ht[i] += std::chrono::duration<double, std::micro>((b_) - (a)).count()
#else
#define HT_T(v) do { } while (0)
#define HT_ACC(i, a, b_) do { } while (0)
#endif
inline double mono_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3; }
inline double trace_us() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)(ts.tv_sec % 1000) * 1e6 + (double)ts.tv_nsec * 1e-3; }
#define TRACE(...) do { if (trace_on()) { fprintf(stderr, "[spl %12.1f] ", trace_us()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); fflush(stderr); } } while (0)
}  // namespace
