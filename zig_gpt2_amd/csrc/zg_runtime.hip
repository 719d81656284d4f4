// zg_runtime.hip — the process runtime behind zg_runtime.h: error text, ctx(), init / shutdown / stream / synchronize, the tensor
// registry, the op tier's staging scope Call with its completion word, and the two caches kept between op-tier calls (the device
// twin of the last in-place elementwise result, the KV-cache mirrors).  Every other unit depends on this one; it launches nothing
// but the completion word's two kernels.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "zg_runtime.h"

namespace zg {

static thread_local char g_err[512] = "";

int decode_paths_off() {
    const char* e = getenv("ZGPT2_DECODE_PATHS_OFF");
    return e ? atoi(e) : 0;
}

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static thread_local char g_kernel[160] = "";
void note_kernel(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_kernel, sizeof(g_kernel), fmt, ap);
    va_end(ap);
}
const char* last_kernel() { return g_kernel; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    set_error("HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
    (void)hipGetLastError();
    return ZG_ERR_HIP;
}

Ctx& ctx() {
    static Ctx c;
    return c;
}

int require_init() {
    ZG_REQUIRE(ctx().inited, ZG_ERR_NOT_INITIALIZED, "zg_init has not been called");
    return ZG_OK;
}

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // plain host memory: not an error for us
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

void Registry::drop_all() {
    for (auto& kv : map) (void)hipFree(kv.second.dev);
    map.clear();
}

// ------------------------------------------------------------------------------------- Shadow
int Shadow::init(size_t cap_bytes) {
    cap = cap_bytes;
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&dev), cap));
    host = static_cast<char*>(malloc(cap));
    ZG_REQUIRE(host != nullptr, ZG_ERR_HIP, "zg_init: out of host memory");
    ptr = nullptr;
    bytes = 0;
    return ZG_OK;
}

void Shadow::release() {
    if (dev) (void)hipFree(dev);
    free(host);
}

float* Shadow::offer(const void* buf, const void* staged, size_t n_bytes) {
    const bool twin = staged != buf && n_bytes <= cap;  // a host buffer: keep a device twin of the result
    ptr = nullptr;
    return twin ? dev : nullptr;
}

void Shadow::keep(const void* buf, size_t n_bytes) {
    memcpy(host, buf, n_bytes);
    ptr = buf;
    bytes = n_bytes;
}

const float* Shadow::match(const void* p, size_t n_bytes) const {
    return p == ptr && n_bytes == bytes && memcmp(p, host, n_bytes) == 0 ? dev : nullptr;
}

// ------------------------------------------------------------------------------------- KvMirrors
int KvMirrors::init(size_t pool_bytes) {
    cap = pool_bytes;
    if (cap > 0) ZG_HIP(hipMalloc(reinterpret_cast<void**>(&pool), cap));
    off = 0;
    return ZG_OK;
}

void KvMirrors::release() {
    map.clear();
    if (pool) (void)hipFree(pool);
}

void KvMirrors::drop_all() {
    map.clear();
    off = 0;
}

// a slot for a cache of seq_len rows: the reference's context (1024 rows) or twice what is needed
static size_t kv_slot_floats(size_t seq_len, size_t E) { return std::max(seq_len * E * 2, (size_t)1024 * E); }

void KvMirrors::make_room(float* const host_cache[2], size_t seq_len, size_t E) {
    size_t need_bytes = 0;
    for (int i = 0; i < 2; ++i) {
        if (is_device_ptr(host_cache[i])) continue;
        auto it = map.find(host_cache[i]);
        if (it == map.end() || it->second.cap_floats < seq_len * E) need_bytes += kv_slot_floats(seq_len, E) * sizeof(float) + 256;
    }
    if (need_bytes > 0 && off > 0 && off + need_bytes > cap && need_bytes <= cap) drop_all();
}

int KvMirrors::attach(float* host_cache, size_t seq_len, size_t E, Call& call, float** dev, KvMirror** mirror) {
    *mirror = nullptr;
    if (is_device_ptr(host_cache)) {
        *dev = host_cache;
        return ZG_OK;
    }
    KvMirror* m = nullptr;
    auto it = map.find(host_cache);
    if (it != map.end()) m = &it->second;
    const size_t need = seq_len * E;
    if (m == nullptr || m->cap_floats < need) {
        const size_t slot = kv_slot_floats(seq_len, E);
        const size_t at = (off + 255) & ~(size_t)255;
        if (pool != nullptr && at + slot * sizeof(float) <= cap) {
            KvMirror fresh;
            fresh.dev = reinterpret_cast<float*>(pool + at);
            fresh.cap_floats = slot;
            fresh.n_embed = E;
            fresh.rows = 0;
            off = at + slot * sizeof(float);
            m = &(map[host_cache] = fresh);  // (an outgrown slot stays behind until zg_unregister_all)
        } else {
            m = nullptr;
            map.erase(host_cache);
        }
    }
    if (m == nullptr)  // pool exhausted: rows 0..T-2 go up, row T-1 comes back, every call
        return call.inout(host_cache, seq_len * E, dev);
    if (m->n_embed != E || m->rows + 1 != seq_len) {
        if (seq_len > 1) ZG_HIP(hipMemcpyAsync(m->dev, host_cache, (seq_len - 1) * E * sizeof(float), hipMemcpyHostToDevice, call.stream()));
        m->n_embed = E;
    }
    m->rows = 0;  // (valid again once this call has succeeded)
    *mirror = m;
    *dev = m->dev;
    return ZG_OK;
}

// ------------------------------------------------------------------------------------- Call
Call::Call() : mark_(ctx().stage.off), pin_mark_(ctx().pin.off), s_(ctx().stream) {}

// A failed call must still release the arenas.
Call::~Call() {
    if (finished_) return;
    (void)hipStreamSynchronize(s_);
    ctx().stage.off = 0;
    ctx().pin.off = 0;
}

int Call::alloc(size_t bytes, void** dev) {
    auto& a = ctx().stage;
    const size_t off = (a.off + 255) & ~(size_t)255;
    ZG_REQUIRE(off + bytes <= a.cap, ZG_ERR_STAGING,
               "host buffers of this call need %zu more bytes than the %zu-byte staging arena "
               "(raise ZGPT2_STAGING_MB / zg_init_ex, pass device pointers, or zg_register_tensor the weights)",
               off + bytes - a.cap, a.cap);
    *dev = a.base + off;
    a.off = off + bytes;
    return ZG_OK;
}

char* Call::pin_alloc(size_t bytes) {  // nullptr: does not fit (the caller takes the pageable path)
    auto& a = ctx().pin;
    const size_t off = (a.off + 255) & ~(size_t)255;
    if (a.base == nullptr || off + bytes > a.cap) return nullptr;
    a.off = off + bytes;
    return a.base + off;
}

size_t Call::arena_left() const {
    const auto& a = ctx().stage;
    const size_t off = (a.off + 255) & ~(size_t)255;
    return off < a.cap ? a.cap - off : 0;
}

// what a kernel may touch in place over PCIe: a few wavefronts' worth of traffic, not a matrix
static constexpr size_t kZeroCopyMax = (size_t)1 << 20;

int Call::stage_in(const void* p, size_t bytes, bool is_param, bool once, const void** dev) {
    if (bytes == 0 || p == nullptr) {
        *dev = p;
        return ZG_OK;
    }
    // Only parameters may come from the registry, and only on an exact (pointer, size) match: the key is a bare
    // host address, and host code frees and reuses addresses (the reference's tests allocate same-sized buffers
    // with page_allocator right after freeing the weights).
    if (is_param) {
        const auto& reg = ctx().registry.map;
        auto it = reg.find(p);
        if (it != reg.end() && it->second.bytes == bytes) {
            *dev = it->second.dev;
            return ZG_OK;
        }
    }
    if (is_device_ptr(p)) {
        *dev = p;
        return ZG_OK;
    }
    // the previous op's result, still on the device?
    if (!is_param && !once)
        if (const float* twin = ctx().shadow.match(p, bytes)) {
            *dev = twin;
            return ZG_OK;
        }
    char* pin = pin_alloc(bytes);
    if (pin != nullptr) {
        memcpy(pin, p, bytes);
        if (once && bytes <= kZeroCopyMax) {
            *dev = pin;
            return ZG_OK;
        }
    }
    void* d = nullptr;
    ZG_TRY(alloc(bytes, &d));
    ZG_HIP(hipMemcpyAsync(d, pin ? pin : p, bytes, hipMemcpyHostToDevice, s_));
    *dev = d;
    return ZG_OK;
}

int Call::stage_out(void* p, size_t bytes, bool copy_in, bool once, void** dev) {
    if (bytes == 0 || p == nullptr) {
        *dev = p;
        return ZG_OK;
    }
    if (is_device_ptr(p)) {
        *dev = p;
        return ZG_OK;
    }
    ZG_REQUIRE(n_outs_ < 24, ZG_ERR_STAGING, "too many staged outputs");
    char* pin = pin_alloc(bytes);
    if (pin != nullptr && copy_in) memcpy(pin, p, bytes);
    if (pin != nullptr && once && bytes <= kZeroCopyMax) {  // the kernel stores straight into the pinned slot
        outs_[n_outs_++] = Out{p, nullptr, pin, bytes};
        *dev = pin;
        return ZG_OK;
    }
    void* d = nullptr;
    ZG_TRY(alloc(bytes, &d));
    if (copy_in) ZG_HIP(hipMemcpyAsync(d, pin ? pin : p, bytes, hipMemcpyHostToDevice, s_));
    outs_[n_outs_++] = Out{p, d, pin, bytes};
    *dev = d;
    return ZG_OK;
}

int Call::also_out(void* host, const void* dev_part, size_t bytes) {
    if (bytes == 0 || host == nullptr || is_device_ptr(host)) return ZG_OK;
    ZG_REQUIRE(n_outs_ < 24, ZG_ERR_STAGING, "too many staged outputs");
    // inside an output that travels through the pinned arena anyway: the CPU copies from there, no second transfer
    const char* d = static_cast<const char*>(dev_part);
    for (int i = 0; i < n_outs_; ++i) {
        const char* base = static_cast<const char*>(outs_[i].dev);
        if (base != nullptr && outs_[i].pin != nullptr && d >= base && d + bytes <= base + outs_[i].bytes) {
            outs_[n_outs_++] = Out{host, nullptr, outs_[i].pin + (d - base), bytes};
            return ZG_OK;
        }
    }
    outs_[n_outs_++] = Out{host, const_cast<void*>(dev_part), pin_alloc(bytes), bytes};
    return ZG_OK;
}

DoneSlot* Call::reserve() {
    auto& w = ctx().done;
    slot_ = DoneSlot{nullptr, 0, false};
    if (w.flag == nullptr || w.calls_since_sync + 1 >= 256) return &slot_;
    for (int i = 0; i < n_outs_; ++i)
        if (outs_[i].dev != nullptr) return &slot_;  // a transfer must follow the kernel: its completion is not the call's
    slot_.flag = w.flag;
    slot_.seq = ++w.seq;
    return &slot_;
}

int Call::finish() {
    Ctx& c = ctx();
    auto& w = c.done;
    const bool poll = w.flag != nullptr && w.calls_since_sync + 1 < 256;
    // Outputs that live in device memory.  A few small ones (the common case: _qkv and _q of an attention call) leave for the pinned
    // arena in the SAME launch that announces the call's completion; anything else by DMA — outputs that lie back to back in both
    // arenas (consecutive out() calls of 256-byte multiples) in one transfer.
    CopySegs segs{};
    size_t seg_bytes = 0;
    bool fused = poll && !slot_.taken;
    for (int i = 0; i < n_outs_ && fused; ++i) {
        if (outs_[i].dev == nullptr) continue;
        if (outs_[i].pin == nullptr || segs.n == 4 || (outs_[i].bytes & 3) || outs_[i].bytes > (64u << 10)) fused = false;
        else {
            segs.src[segs.n] = outs_[i].dev;
            segs.dst[segs.n] = outs_[i].pin;
            segs.bytes[segs.n++] = (unsigned)outs_[i].bytes;
            seg_bytes += outs_[i].bytes;
        }
    }
    fused = fused && segs.n > 0 && seg_bytes <= (64u << 10);
    if (!fused)
        for (int i = 0; i < n_outs_; ++i) {
            if (outs_[i].dev == nullptr) continue;
            size_t bytes = outs_[i].bytes;
            int j = i;
            while (outs_[i].pin != nullptr && j + 1 < n_outs_ && outs_[j + 1].dev != nullptr && outs_[j + 1].pin != nullptr &&
                   static_cast<char*>(outs_[i].dev) + bytes == static_cast<char*>(outs_[j + 1].dev) && outs_[i].pin + bytes == outs_[j + 1].pin) {
                bytes += outs_[j + 1].bytes;
                ++j;
            }
            ZG_HIP(hipMemcpyAsync(outs_[i].pin ? (void*)outs_[i].pin : outs_[i].host, outs_[i].dev, bytes, hipMemcpyDeviceToHost, s_));
            i = j;
        }
    // Op-tier calls are synchronous on return: the reference's host code reads the buffers next.  The host polls a pinned
    // completion word stored in stream order behind the call's work (cheaper than the runtime's wake-up); every 256th call —
    // and any call whose word does not arrive — drains the stream the ordinary way, which also surfaces asynchronous errors.
    bool drained = false, polled = false;
    if (w.flag != nullptr && ++w.calls_since_sync < 256) {
        // (a reserved sequence number no launch took is simply skipped: the next one is larger)
        const bool own = slot_.taken;
        const unsigned seq = own ? slot_.seq : ++w.seq;
        const int st = own ? ZG_OK : fused ? launch_copy_out_done(segs, w.flag, seq, s_) : launch_done_flag(w.flag, seq, s_);
        polled = st == ZG_OK;
        if (st == ZG_OK)
            for (long spins = 0; spins < (1L << 24) && !drained; ++spins) {
                drained = __atomic_load_n(w.flag, __ATOMIC_ACQUIRE) == seq;
                if (!drained) __builtin_ia32_pause();
            }
        else if (fused)
            return st;  // (the outputs have not left: the call failed)
    }
    if (!drained) {
        if (polled) ++w.missed;
        ZG_HIP(hipStreamSynchronize(s_));
        w.calls_since_sync = 0;
    }
    for (int i = 0; i < n_outs_; ++i)
        if (outs_[i].pin != nullptr) memcpy(outs_[i].host, outs_[i].pin, outs_[i].bytes);
    c.stage.off = mark_;
    c.pin.off = pin_mark_;
    n_outs_ = 0;
    slot_ = DoneSlot{nullptr, 0, false};
    finished_ = true;
    return ZG_OK;
}

}  // namespace zg

using namespace zg;

extern "C" {

const char* zg_last_error(void) { return zg::g_err; }

// (at_least: the smallest value the variable may set; anything below it, or no number, leaves the default)
static size_t env_mb(const char* name, size_t dflt, long at_least = 0) {
    if (const char* e = getenv(name)) {
        const long v = atol(e);
        if (v >= at_least) return (size_t)v;
    }
    return dflt;
}

int zg_init_ex(int device, size_t staging_bytes) {
    Ctx& c = ctx();
    if (c.inited) {
        ZG_REQUIRE(c.device == device, ZG_ERR_ARG, "already initialised on device %d", c.device);
        return ZG_OK;
    }
    int n = 0;
    ZG_HIP(hipGetDeviceCount(&n));
    ZG_REQUIRE(device >= 0 && device < n, ZG_ERR_ARG, "device %d out of range (%d visible)", device, n);
    ZG_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    ZG_HIP(hipGetDeviceProperties(&prop, device));
    ZG_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, ZG_ERR_UNSUPPORTED,
               "libzgpt2_hip is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
    ZG_HIP(hipStreamCreateWithFlags(&c.own_stream, hipStreamNonBlocking));
    c.stream = c.own_stream;
    c.stage.cap = staging_bytes;
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.stage.base), c.stage.cap));
    // pinned twin of the staging arena for the small host buffers of src/main.zig's State (a few KB each; the logits 200 KB)
    c.pin.cap = std::min(staging_bytes, env_mb("ZGPT2_PINNED_MB", 32) << 20);
    if (c.pin.cap > 0) ZG_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.pin.base), c.pin.cap, hipHostMallocDefault));
    c.pin.off = 0;
    // device pool for the mirrors of caller-owned KV caches (zg_attn_forward): 124M needs 75 MB, GPT-2 XL 630 MB of 288 GB
    ZG_TRY(c.mirrors.init(env_mb("ZGPT2_KV_MIRROR_MB", 1024) << 20));
    ZG_TRY(c.shadow.init((size_t)1 << 20));
    ZG_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.d_flag), 64, hipHostMallocDefault));
    *c.d_flag = 0;
    c.done.flag = reinterpret_cast<unsigned*>(c.d_flag) + 8;
    *c.done.flag = 0;
    c.done.seq = c.done.calls_since_sync = 0;
    if (env_mb("ZGPT2_OP_POLL", 1) == 0) c.done.flag = nullptr;  // measurement switch: drain every op-tier call with hipStreamSynchronize
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.d_zero), 64));
    ZG_HIP(hipMemset(c.d_zero, 0, 64));
    c.attn_part.floats = (size_t)4 << 20;
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.attn_part.buf), c.attn_part.floats * sizeof(float)));
    c.stage.off = 0;
    c.device = device;
    c.inited = true;
    return ZG_OK;
}

int zg_init(int device) { return zg_init_ex(device, env_mb("ZGPT2_STAGING_MB", 512, 1) << 20); }

int zg_shutdown(void) {
    Ctx& c = ctx();
    if (!c.inited) return ZG_OK;
    (void)hipStreamSynchronize(c.stream);
    c.registry.drop_all();
    (void)hipFree(c.stage.base);
    if (c.pin.base) (void)hipHostFree(c.pin.base);
    c.mirrors.release();
    c.shadow.release();
    (void)hipHostFree(c.d_flag);
    (void)hipFree(c.d_zero);
    (void)hipFree(c.attn_part.buf);
    (void)hipStreamDestroy(c.own_stream);
    c = Ctx();
    return ZG_OK;
}

int zg_set_stream(void* hip_stream) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    c.stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : c.own_stream;
    return ZG_OK;
}

int zg_synchronize(void) {
    ZG_TRY(require_init());
    ZG_HIP(hipStreamSynchronize(ctx().stream));
    return ZG_OK;
}

int zg_register_tensor(const float* host_ptr, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(host_ptr && len, ZG_ERR_ARG, "zg_register_tensor: null/empty tensor");
    auto& reg = ctx().registry.map;
    if (is_device_ptr(host_ptr)) return ZG_OK;
    auto it = reg.find(host_ptr);
    if (it != reg.end()) {
        (void)hipFree(it->second.dev);
        reg.erase(it);
    }
    void* d = nullptr;
    ZG_HIP(hipMalloc(&d, len * sizeof(float)));
    ZG_HIP(hipMemcpy(d, host_ptr, len * sizeof(float), hipMemcpyHostToDevice));
    reg[host_ptr] = Registered{d, len * sizeof(float)};
    return ZG_OK;
}

int zg_unregister_tensor(const float* host_ptr) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    c.mirrors.drop(host_ptr);  // (a KV-cache mirror keyed by this address)
    auto it = c.registry.map.find(host_ptr);
    if (it == c.registry.map.end()) return ZG_OK;  // never registered (or a device pointer): nothing to drop
    ZG_HIP(hipStreamSynchronize(c.stream));
    (void)hipFree(it->second.dev);
    c.registry.map.erase(it);
    return ZG_OK;
}

int zg_unregister_all(void) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    c.registry.drop_all();
    c.mirrors.drop_all();
    return ZG_OK;
}

// The op tier's completion word in front of its wrap / what became of it (tests; include/zgpt2.h).  The library stream is drained
// first: no call is in flight whose number the word still has to take.
int zg_debug_ops_set_done_seq(unsigned seq) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    c.done.seq = seq;
    return ZG_OK;
}
int zg_debug_ops_done_state(unsigned long long* out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(out && n_out >= 3, ZG_ERR_ARG, "ops_done_state: need 3 words");
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    out[0] = c.done.seq;
    out[1] = c.done.flag ? __atomic_load_n(c.done.flag, __ATOMIC_ACQUIRE) : 0u;
    out[2] = c.done.missed;
    return ZG_OK;
}

}  // extern "C"
