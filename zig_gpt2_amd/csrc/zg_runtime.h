// zg_runtime.h — process-wide runtime of libzgpt2_hip (zg_runtime.hip): device and stream, the tensor registry, the op tier's
// staging scope with its two arenas and its completion word, and the two caches kept between op-tier calls.
#pragma once
#include <unordered_map>

#include "zg_kernels.h"

namespace zg {

class Call;

struct Registered {
    void* dev;
    size_t bytes;
};

// zg_register_tensor's device copies of host parameters, keyed by host address.  Written by the registry entry points
// (zg_runtime.hip); read by Call::stage_in for parameters only.
struct Registry {
    std::unordered_map<const void*, Registered> map;
    void drop_all();  // frees every device copy (the caller has drained the stream)
};

// Device mirror of a caller-owned host KV cache (zg_attn_forward, ops.zig:129-173): the caller appends one row per call and
// never reads the cache itself, so the rows it handed over once stay on the device (keyed by the cache's host address).
struct KvMirror {
    float* dev = nullptr;
    size_t cap_floats = 0;
    size_t n_embed = 0;
    size_t rows = 0;  // rows 0 .. rows-1 of the mirror equal the caller's cache
};

// The mirrors and the device pool they live in (allocated in zg_init: no forward allocates).  The pool is a bump allocator.
// Written by its own functions only; zg_attn_forward commits `rows` of the mirrors attach() handed it once its call has succeeded.
struct KvMirrors {
    char* pool = nullptr;
    size_t cap = 0;
    size_t off = 0;
    std::unordered_map<const void*, KvMirror> map;
    int init(size_t pool_bytes);
    void release();
    // Mirrors of caches the caller has long freed stay in the pool.  When the two caches of a call would not fit what is left, every
    // mirror is dropped and the pool starts over (the live caches upload once more at their next call) — before attach() takes
    // any pointer into the map.
    void make_room(float* const host_cache[2], size_t seq_len, size_t E);
    // One cache of a zg_attn_forward call at position seq_len: *dev is what the kernels read and append to — the pointer itself
    // (device memory), its mirror (*mirror set; rows 0 .. seq_len-2 uploaded unless this call continues the sequence the mirror
    // holds), or, with no room in the pool, the whole cache staged through `call`.
    int attach(float* host_cache, size_t seq_len, size_t E, Call& call, float** dev, KvMirror** mirror);
    void drop(const void* host_cache) { map.erase(host_cache); }  // the next zg_attn_forward uploads the cache again
    void drop_all();  // the pool empties when every mirror is gone
};

// The result of the last in-place elementwise op on a HOST buffer, kept twice: in device memory (what the next Linear reads
// instead of uploading the same bytes again — in src/main.zig every Linear's input is the previous op's output) and in host
// memory (what the caller's buffer is compared with before the device twin is trusted).  Written by offer / keep only
// (zg_layernorm_forward, zg_gelu); read by Call::stage_in through match.
struct Shadow {
    float* dev = nullptr;
    char* host = nullptr;
    size_t cap = 0;
    const void* ptr = nullptr;
    size_t bytes = 0;
    int init(size_t cap_bytes);
    void release();
    // In front of the launch: the twin held so far is no longer valid; returns where the kernel stores the new one, or nullptr
    // (the buffer was not staged — a device pointer — or is larger than the twin).
    float* offer(const void* buf, const void* staged, size_t n_bytes);
    // Behind a finish() that succeeded, for a buffer offer() returned a twin for: the caller's bytes are the twin's from here on.
    void keep(const void* buf, size_t n_bytes);
    // The device twin of exactly these bytes (same buffer, same length, and the caller has not changed a byte of it), or nullptr.
    const float* match(const void* p, size_t n_bytes) const;
};

struct Ctx {
    // zg_init_ex / zg_shutdown / zg_set_stream; read by every unit
    bool inited = false;
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // the stream every launch uses (own_stream unless zg_set_stream)
    // device staging arena for host-pointer callers (op tier).  off: Call (alloc, finish, ~Call).  The model tier's uploads
    // (api_gpt.hip) pass through base .. base + cap between calls.
    struct {
        char* base = nullptr;
        size_t cap = 0;
        size_t off = 0;
    } stage;
    // pinned host arena of the op tier: the caller's pageable buffers are copied here by the CPU, and the GPU either reads /
    // writes this memory in place (buffers a kernel touches once) or moves it with ONE asynchronous DMA each way.
    // off: Call (pin_alloc, finish, ~Call)
    struct {
        char* base = nullptr;
        size_t cap = 0;
        size_t off = 0;
    } pin;
    KvMirrors mirrors;
    Shadow shadow;
    // the completion word of op-tier calls.  Call (reserve, finish); seq also zg_debug_ops_set_done_seq
    struct {
        unsigned* flag = nullptr;  // pinned completion word of op-tier calls (d_flag + 8), its sequence number, calls since a real drain
        unsigned seq = 0;
        unsigned calls_since_sync = 0;
        unsigned long long missed = 0;  // calls that polled to the end without seeing their number and drained the stream (zg_debug_ops_done_state)
    } done;
    // zg_init_ex; read by the op tier, the kernels' launchers and the model tier
    int* d_flag = nullptr;    // pinned host int the kernels raise for index-range checks (read after the call's drain)
    float* d_zero = nullptr;  // 64 zero bytes (stand-in operand for absent bias / residual)
    // op-tier attention partials (sized at init).  zg_init_ex; the kernels of attn_core (api_ops.hip) write through it
    struct {
        float* buf = nullptr;
        size_t floats = 0;
    } attn_part;
    Registry registry;
    unsigned long long* dbg = nullptr;  // -DZG_STAMPS diagnostic buffer (the model tier's debug unit)
};

Ctx& ctx();
int require_init();
bool is_device_ptr(const void* p);

// Per-call staging scope for the op tier.  Device pointers pass through untouched.  Host pointers:
//   in / out / inout      the buffer must live in device memory while the kernels run (read by many workgroups, or read back):
//                         CPU copy into the pinned arena, one asynchronous DMA into the device arena (and back at finish)
//   *_once                a kernel reads / writes every element ONCE: the kernel works on the pinned arena in place (PCIe
//                         zero-copy), no DMA at all — the common case for the small activation vectors of src/main.zig:119-195
// Buffers that do not fit the pinned arena go through hipMemcpyAsync on the caller's pageable memory, as before.
// A scope that ends without a finish() that succeeded — the call failed — drains the stream and empties both arenas.
class Call {
  public:
    Call();
    ~Call();
    Call(const Call&) = delete;
    Call& operator=(const Call&) = delete;
    // Activations (inputs, indices, q / k / v): always the caller's bytes of THIS call.
    template <typename T>
    int in(const T* p, size_t n, const T** dev) {
        return stage_in(p, n * sizeof(T), false, false, reinterpret_cast<const void**>(dev));
    }
    template <typename T>
    int in_once(const T* p, size_t n, const T** dev) {
        return stage_in(p, n * sizeof(T), false, true, reinterpret_cast<const void**>(dev));
    }
    // Borrowed parameters (weights, biases, LayerNorm vectors): a zg_register_tensor mirror of exactly this
    // pointer AND size is used instead of staging; anything else is staged like an activation.
    template <typename T>
    int param(const T* p, size_t n, const T** dev) {
        return stage_in(p, n * sizeof(T), true, false, reinterpret_cast<const void**>(dev));
    }
    // Device scratch from the same arena (released by finish()).
    template <typename T>
    int scratch(size_t n, T** dev) {
        return alloc(n * sizeof(T), reinterpret_cast<void**>(dev));
    }
    size_t arena_left() const;
    template <typename T>
    int out(T* p, size_t n, T** dev) {
        return stage_out(p, n * sizeof(T), false, false, reinterpret_cast<void**>(dev));
    }
    template <typename T>
    int out_once(T* p, size_t n, T** dev) {
        return stage_out(p, n * sizeof(T), false, true, reinterpret_cast<void**>(dev));
    }
    template <typename T>
    int inout(T* p, size_t n, T** dev) {
        return stage_out(p, n * sizeof(T), true, false, reinterpret_cast<void**>(dev));
    }
    template <typename T>
    int inout_once(T* p, size_t n, T** dev) {
        return stage_out(p, n * sizeof(T), true, true, reinterpret_cast<void**>(dev));
    }
    // A second host destination for a part of an output already staged with out() (the cache rows inside _qkv).
    int also_out(void* host, const void* dev_part, size_t bytes);
    // A call whose LAST kernel is a single workgroup writing zero-copy outputs may let that kernel store the completion word
    // itself: reserve() offers that launch the word and the sequence number finish() will poll for (flag == nullptr: not available —
    // polling is off, the periodic real drain is due, or an output of this call still needs a DMA behind the kernel); a launch
    // that sets `taken` tells finish() that the kernel stores the word, so the one-thread launch is skipped.
    DoneSlot* reserve();
    // Copies outputs back (if any were staged), synchronises the stream, releases the arenas.
    int finish();
    hipStream_t stream() const { return s_; }

  private:
    int stage_in(const void* p, size_t bytes, bool is_param, bool once, const void** dev);
    int stage_out(void* p, size_t bytes, bool copy_in, bool once, void** dev);
    int alloc(size_t bytes, void** dev);
    char* pin_alloc(size_t bytes);
    struct Out {
        void* host;
        void* dev;   // device buffer to copy from (nullptr: the pinned slot already holds the result)
        char* pin;   // pinned slot (nullptr: pageable path, straight into host)
        size_t bytes;
    };
    Out outs_[24];
    int n_outs_ = 0;
    DoneSlot slot_{nullptr, 0, false};
    bool finished_ = false;
    size_t mark_, pin_mark_;
    hipStream_t s_;
};

}  // namespace zg
