// api_ops.hip — runtime + op tier of the C ABI (include/zgpt2.h): one entry point per public decl
// of the reference's src/ops.zig, same argument meaning, Zig slices passed as (ptr, len).
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

// ------------------------------------------------------------------------------------- Call
Call::Call() : mark_(ctx().stage_off), pin_mark_(ctx().pin_off), s_(ctx().stream) {}

int Call::alloc(size_t bytes, void** dev) {
    Ctx& c = ctx();
    const size_t off = (c.stage_off + 255) & ~(size_t)255;
    ZG_REQUIRE(off + bytes <= c.stage_cap, ZG_ERR_STAGING,
               "host buffers of this call need %zu more bytes than the %zu-byte staging arena "
               "(raise ZGPT2_STAGING_MB / zg_init_ex, pass device pointers, or zg_register_tensor the weights)",
               off + bytes - c.stage_cap, c.stage_cap);
    *dev = c.stage + off;
    c.stage_off = off + bytes;
    return ZG_OK;
}

char* Call::pin_alloc(size_t bytes) {  // nullptr: does not fit (the caller takes the pageable path)
    Ctx& c = ctx();
    const size_t off = (c.pin_off + 255) & ~(size_t)255;
    if (c.pin == nullptr || off + bytes > c.pin_cap) return nullptr;
    c.pin_off = off + bytes;
    return c.pin + off;
}

size_t Call::arena_left() const {
    const Ctx& c = ctx();
    const size_t off = (c.stage_off + 255) & ~(size_t)255;
    return off < c.stage_cap ? c.stage_cap - off : 0;
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
        auto it = ctx().registry.find(p);
        if (it != ctx().registry.end() && it->second.bytes == bytes) {
            *dev = it->second.dev;
            return ZG_OK;
        }
    }
    if (is_device_ptr(p)) {
        *dev = p;
        return ZG_OK;
    }
    {   // the previous op's result, still on the device?  (same buffer, same length, and the caller has not changed a byte of it)
        Ctx& c = ctx();
        if (!is_param && !once && p == c.shadow_ptr && bytes == c.shadow_bytes && memcmp(p, c.shadow_host, bytes) == 0) {
            *dev = c.shadow_dev;
            return ZG_OK;
        }
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

void Call::reserve(unsigned** flag, unsigned* seq) {
    Ctx& c = ctx();
    *flag = nullptr;
    *seq = 0;
    if (c.done_flag == nullptr || c.calls_since_sync + 1 >= 256) return;
    for (int i = 0; i < n_outs_; ++i)
        if (outs_[i].dev != nullptr) return;  // a transfer must follow the kernel: its completion is not the call's
    reserved_seq_ = ++c.done_seq;
    reserved_ = true;
    *flag = c.done_flag;
    *seq = reserved_seq_;
}

int Call::finish() {
    Ctx& c = ctx();
    const bool poll = c.done_flag != nullptr && c.calls_since_sync + 1 < 256;
    // Outputs that live in device memory.  A few small ones (the common case: _qkv and _q of an attention call) leave for the pinned
    // arena in the SAME launch that announces the call's completion; anything else by DMA — outputs that lie back to back in both
    // arenas (consecutive out() calls of 256-byte multiples) in one transfer.
    CopySegs segs{};
    size_t seg_bytes = 0;
    bool fused = poll && !(reserved_ && announced_);
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
    if (c.done_flag != nullptr && ++c.calls_since_sync < 256) {
        // (a reserved sequence number nobody announced is simply skipped: the next one is larger)
        const bool own = reserved_ && announced_;
        const unsigned seq = own ? reserved_seq_ : ++c.done_seq;
        const int st = own ? ZG_OK : fused ? launch_copy_out_done(segs, c.done_flag, seq, s_) : launch_done_flag(c.done_flag, seq, s_);
        polled = st == ZG_OK;
        if (st == ZG_OK)
            for (long spins = 0; spins < (1L << 24) && !drained; ++spins) {
                drained = __atomic_load_n(c.done_flag, __ATOMIC_ACQUIRE) == seq;
                if (!drained) __builtin_ia32_pause();
            }
        else if (fused)
            return st;  // (the outputs have not left: the call failed)
    }
    if (!drained) {
        if (polled) ++c.done_missed;
        ZG_HIP(hipStreamSynchronize(s_));
        c.calls_since_sync = 0;
    }
    for (int i = 0; i < n_outs_; ++i)
        if (outs_[i].pin != nullptr) memcpy(outs_[i].host, outs_[i].pin, outs_[i].bytes);
    c.stage_off = mark_;
    c.pin_off = pin_mark_;
    n_outs_ = 0;
    reserved_ = announced_ = false;
    return ZG_OK;
}

// A failed call must still release the arenas.
struct CallGuard {
    Call& c;
    bool done = false;
    explicit CallGuard(Call& cc) : c(cc) {}
    ~CallGuard() {
        if (!done) {
            (void)hipStreamSynchronize(c.stream());
            ctx().stage_off = 0;
            ctx().pin_off = 0;
        }
    }
};

// Linear.forward for batch >= 16 on the matrix cores (ops.zig:21-46 with M = inputs.len / in_features, :22).
// The op tier is fp32 in, fp32 out, arbitrary fp32 weights: both operands are split EXACTLY into three bf16
// planes (x = hi + mid + lo, 3 x 8 mantissa bits) and the GEMM sums the six plane products whose weight is
// above 2^-24 of the leading one — every bf16 x bf16 product is exact in fp32 and accumulation is fp32, i.e. the
// result is fp32-sgemm grade (measured against the oracle at the reference's tolerance in the tests).
// Order: small products first.
static bool linear_mfma_ok(size_t in_f, size_t out_f, size_t m, size_t arena_left) {
    if (m < 16 || in_f < 128 || in_f % 64 != 0) return false;
    if (m * in_f * 3 >= (1u << 30) || out_f * in_f * 3 >= (1u << 30)) return false;
    // a ragged width (out_f % 4 != 0) is stored by the four-wave GEMM only, whose packed arguments end at K = 16384 per plane
    // and rows of 65535 elements (three planes side by side): such a Linear stays on the GEMV kernels
    if (out_f % 4 != 0 && (in_f * 3 >= 65536 || in_f / 64 >= 256)) return false;
    return (m + out_f) * in_f * 3 * sizeof(bf16_t) + 1024 <= arena_left;
}

static int linear_mfma(Call& call, size_t in_f, size_t out_f, const float* w, const float* bias, const float* x,
                       size_t m, float* y) {
    bf16_t *xp, *wp;
    ZG_TRY(call.scratch(m * in_f * 3, &xp));
    ZG_TRY(call.scratch(out_f * in_f * 3, &wp));
    ZG_TRY(launch_split3(x, m, (int)in_f, xp, call.stream()));
    ZG_TRY(launch_split3(w, out_f, (int)in_f, wp, call.stream()));
    GemmPlanes pl{};
    pl.lda = pl.ldb = (int)(3 * in_f);
    pl.kpp = (int)(in_f / 64);
    pl.npairs = 6;  // (x plane, w plane): lo*hi, mid*mid, hi*lo, mid*hi, hi*mid, hi*hi
    pl.pa_bits = 0x001012u;
    pl.pb_bits = 0x010210u;
    return launch_gemm_planes(xp, wp, bias, y, (int)m, (int)out_f, pl, (int)out_f, false, false, call.stream());
}

static int linear_device(size_t in_f, size_t out_f, const float* w, const float* bias, const float* x,
                         size_t m, float* y, hipStream_t s) {
    if (m == 0 || out_f == 0) return ZG_OK;
    ZG_REQUIRE(in_f > 0 && in_f <= 8192, ZG_ERR_UNSUPPORTED, "Linear: in_features %zu outside 1..8192", in_f);
    size_t mb = 8;
    while (mb > 1 && (mb * in_f + 8 * mb + 64) * sizeof(float) > 160 * 1024) mb >>= 1;
    for (size_t m0 = 0; m0 < m; m0 += mb) {
        GemvArgs a{};
        a.W = w;
        a.bias = bias;
        a.N = (int)out_f;
        a.K = (int)in_f;
        a.M = (int)((m - m0 < mb) ? (m - m0) : mb);
        a.prologue = PRO_NONE;
        a.epilogue = EPI_STORE;
        a.x = x + m0 * in_f;
        a.x_stride = (int)in_f;
        a.y = y + m0 * out_f;
        a.y_stride = (int)out_f;
        a.zero = ctx().d_zero;
        ZG_TRY(launch_gemv(a, gemv_plan(a, WT_F32), WT_F32, s));
    }
    return ZG_OK;
}

// Linear.forward has no size limit (src/ops.zig:21-46).  The GEMV kernels keep a batch of input rows in LDS, which ends at
// in_features = 8192: a wider Linear runs as K chunks of <= 8192 — chunk 0 computes y = bias + W[:, chunk] x[chunk], every
// later chunk adds its product to y (the residual epilogue, y aliasing the residual) — over contiguous copies of the chunk's
// columns of W (blocks of rows, so that the copy stays a few tens of MB of the staging arena) and of x.  fp32 throughout; the
// partial sums of a row meet in chunk order.
static int linear_device_wide(Call& call, size_t in_f, size_t out_f, const float* w, const float* bias, const float* x, size_t m, float* y) {
    hipStream_t s = call.stream();
    if (in_f <= 8192) return linear_device(in_f, out_f, w, bias, x, m, y, s);
    if (m == 0 || out_f == 0) return ZG_OK;
    const size_t kc_max = 8192;
    size_t rows = (((size_t)64 << 20) / (kc_max * sizeof(float)));  // rows of W per block: 64 MiB of chunk copy
    if (rows > out_f) rows = out_f;
    float *wc, *xc;
    ZG_TRY(call.scratch(rows * kc_max, &wc));
    ZG_TRY(call.scratch(8 * kc_max, &xc));
    for (size_t m0 = 0; m0 < m; m0 += 8) {
        const size_t mb = m - m0 < 8 ? m - m0 : 8;
        // (the ragged chunk goes FIRST: only the plain store epilogue of the GEMV kernels takes a K that is not a multiple of 8,
        // the accumulating chunks behind it are whole — tools/fuzz_ops.py found in_features = 8192 j + 579 failing the other way round)
        const size_t first = in_f % kc_max ? in_f % kc_max : kc_max;
        for (size_t k0 = 0; k0 < in_f; k0 += (k0 == 0 ? first : kc_max)) {
            const size_t kc = k0 == 0 ? first : kc_max;
            ZG_HIP(hipMemcpy2DAsync(xc, kc * 4, x + m0 * in_f + k0, in_f * 4, kc * 4, mb, hipMemcpyDeviceToDevice, s));
            for (size_t n0 = 0; n0 < out_f; n0 += rows) {
                const size_t nb = out_f - n0 < rows ? out_f - n0 : rows;
                ZG_HIP(hipMemcpy2DAsync(wc, kc * 4, w + n0 * in_f + k0, in_f * 4, kc * 4, nb, hipMemcpyDeviceToDevice, s));
                GemvArgs a{};
                a.W = wc;
                a.bias = (k0 == 0 && bias) ? bias + n0 : nullptr;
                a.N = (int)nb;
                a.K = (int)kc;
                a.M = (int)mb;
                a.prologue = PRO_NONE;
                a.epilogue = k0 == 0 ? EPI_STORE : EPI_RESIDUAL;
                a.x = xc;
                a.x_stride = (int)kc;
                a.y = y + m0 * out_f + n0;
                a.y_stride = (int)out_f;
                a.resid = k0 == 0 ? nullptr : a.y;
                a.resid_stride = (int)out_f;
                a.zero = ctx().d_zero;
                ZG_TRY(launch_gemv(a, gemv_plan(a, WT_F32), WT_F32, s));
            }
        }
    }
    return ZG_OK;
}

static int attn_core(const float* q, const float* k, const float* v, long stride_b, long stride_h,
                     long stride_t, size_t batch, size_t n_heads, size_t seq_len, float* out, hipStream_t s, size_t head_dim = 64) {
    Ctx& c = ctx();
    if (batch == 0 || n_heads == 0) return ZG_OK;  // k.len below one sequence: the reference's loop over the batch does nothing (ops.zig:259-261)
    const int splits = (int)((seq_len + kAttnChunk - 1) / kAttnChunk);
    // (a shape whose split partials do not fit the op tier's buffer — very long sequences x many heads — takes the general kernel too)
    if (head_dim != 64 || batch * n_heads * splits * kPartStride > c.attn_part_floats)
        return launch_attn_any_dim(q, k, v, stride_b, stride_h, stride_t, (int)batch, (int)n_heads, (int)head_dim, (int)seq_len, out, s);
    AttnArgs a{};
    a.q = q;
    a.k = k;
    a.v = v;
    a.stride_b = stride_b;
    a.stride_h = stride_h;
    a.stride_t = stride_t;
    a.n_heads = (int)n_heads;
    a.head_dim = 64;
    a.batch = (int)batch;
    a.ctrl = nullptr;
    a.seq_len = (int)seq_len;
    a.t_hi = (int)seq_len;
    a.max_splits = splits;
    a.part = c.attn_part;
    ZG_TRY(launch_attn_decode(a, s));
    return launch_attn_merge(c.attn_part, (int)batch, (int)n_heads, 64, splits, (int)seq_len, out, s);
}

}  // namespace zg

using namespace zg;

extern "C" {

const char* zg_last_error(void) { return zg::g_err; }

static size_t env_mb(const char* name, size_t dflt) {
    if (const char* e = getenv(name)) {
        const long v = atol(e);
        if (v >= 0) return (size_t)v;
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
    c.stage_cap = staging_bytes;
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.stage), c.stage_cap));
    // pinned twin of the staging arena for the small host buffers of src/main.zig's State (a few KB each; the logits 200 KB)
    c.pin_cap = std::min(staging_bytes, env_mb("ZGPT2_PINNED_MB", 32) << 20);
    if (c.pin_cap > 0) ZG_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.pin), c.pin_cap, hipHostMallocDefault));
    c.pin_off = 0;
    // device pool for the mirrors of caller-owned KV caches (zg_attn_forward): 124M needs 75 MB, GPT-2 XL 630 MB of 288 GB
    c.kv_pool_cap = env_mb("ZGPT2_KV_MIRROR_MB", 1024) << 20;
    if (c.kv_pool_cap > 0) ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.kv_pool), c.kv_pool_cap));
    c.kv_pool_off = 0;
    c.shadow_cap = (size_t)1 << 20;
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.shadow_dev), c.shadow_cap));
    c.shadow_host = static_cast<char*>(malloc(c.shadow_cap));
    ZG_REQUIRE(c.shadow_host != nullptr, ZG_ERR_HIP, "zg_init: out of host memory");
    c.shadow_ptr = nullptr;
    c.shadow_bytes = 0;
    ZG_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.d_flag), 64, hipHostMallocDefault));
    *c.d_flag = 0;
    c.done_flag = reinterpret_cast<unsigned*>(c.d_flag) + 8;
    *c.done_flag = 0;
    c.done_seq = c.calls_since_sync = 0;
    if (env_mb("ZGPT2_OP_POLL", 1) == 0) c.done_flag = nullptr;  // measurement switch: drain every op-tier call with hipStreamSynchronize
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.d_zero), 64));
    ZG_HIP(hipMemset(c.d_zero, 0, 64));
    c.attn_part_floats = (size_t)4 << 20;
    ZG_HIP(hipMalloc(reinterpret_cast<void**>(&c.attn_part), c.attn_part_floats * sizeof(float)));
    c.stage_off = 0;
    c.device = device;
    c.inited = true;
    return ZG_OK;
}

int zg_init(int device) {
    size_t mb = 512;
    if (const char* e = getenv("ZGPT2_STAGING_MB")) {
        const long v = atol(e);
        if (v > 0) mb = (size_t)v;
    }
    return zg_init_ex(device, mb << 20);
}

int zg_shutdown(void) {
    Ctx& c = ctx();
    if (!c.inited) return ZG_OK;
    (void)hipStreamSynchronize(c.stream);
    for (auto& kv : c.registry) (void)hipFree(kv.second.dev);
    c.registry.clear();
    c.kv_mirrors.clear();
    (void)hipFree(c.stage);
    if (c.pin) (void)hipHostFree(c.pin);
    if (c.kv_pool) (void)hipFree(c.kv_pool);
    if (c.shadow_dev) (void)hipFree(c.shadow_dev);
    free(c.shadow_host);
    (void)hipHostFree(c.d_flag);
    (void)hipFree(c.d_zero);
    (void)hipFree(c.attn_part);
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
    Ctx& c = ctx();
    if (is_device_ptr(host_ptr)) return ZG_OK;
    auto it = c.registry.find(host_ptr);
    if (it != c.registry.end()) {
        (void)hipFree(it->second.dev);
        c.registry.erase(it);
    }
    void* d = nullptr;
    ZG_HIP(hipMalloc(&d, len * sizeof(float)));
    ZG_HIP(hipMemcpy(d, host_ptr, len * sizeof(float), hipMemcpyHostToDevice));
    c.registry[host_ptr] = Registered{d, len * sizeof(float)};
    return ZG_OK;
}

int zg_unregister_tensor(const float* host_ptr) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    c.kv_mirrors.erase(host_ptr);  // (a KV-cache mirror keyed by this address: the next zg_attn_forward uploads the cache again)
    auto it = c.registry.find(host_ptr);
    if (it == c.registry.end()) return ZG_OK;  // never registered (or a device pointer): nothing to drop
    ZG_HIP(hipStreamSynchronize(c.stream));
    (void)hipFree(it->second.dev);
    c.registry.erase(it);
    return ZG_OK;
}

int zg_unregister_all(void) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    for (auto& kv : c.registry) (void)hipFree(kv.second.dev);
    c.registry.clear();
    c.kv_mirrors.clear();
    c.kv_pool_off = 0;  // the pool is a bump allocator: it empties when every mirror is gone
    return ZG_OK;
}

// ------------------------------------------------------------------------------ Linear
int zg_linear_forward(size_t in_features, size_t out_features, const float* weight,
                      const float* bias_or_null, const float* inputs, size_t inputs_len,
                      float* outputs, size_t outputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(in_features > 0 && weight && (inputs || inputs_len == 0), ZG_ERR_ARG, "Linear: null argument");
    const size_t batch = inputs_len / in_features;  // ops.zig:22
    ZG_REQUIRE(outputs || batch * out_features == 0, ZG_ERR_ARG, "Linear: null outputs");
    ZG_REQUIRE(inputs_len == batch * in_features, ZG_ERR_SHAPE,
               "Linear: inputs.len %zu is not a multiple of in_features %zu", inputs_len, in_features);
    ZG_REQUIRE(outputs_len >= batch * out_features, ZG_ERR_SHAPE,
               "Linear: outputs.len %zu < batch %zu * out_features %zu", outputs_len, batch, out_features);
    Call call;
    CallGuard guard(call);
    const float *w, *b, *x;
    float* y;
    ZG_TRY(call.param(weight, in_features * out_features, &w));
    ZG_TRY(call.param(bias_or_null, out_features, &b));
    ZG_TRY(call.in(inputs, inputs_len, &x));  // (read by every workgroup: device memory)
    if (in_features <= 8192) ZG_TRY(call.out_once(outputs, batch * out_features, &y));  // every element stored once
    else ZG_TRY(call.out(outputs, batch * out_features, &y));                          // K chunks accumulate into y
    if (linear_mfma_ok(in_features, out_features, batch, call.arena_left()))
        ZG_TRY(linear_mfma(call, in_features, out_features, w, b, x, batch, y));
    else
        ZG_TRY(linear_device_wide(call, in_features, out_features, w, b, x, batch, y));
    ZG_TRY(call.finish());
    guard.done = true;
    return ZG_OK;
}

// ------------------------------------------------------------------------------ MFMA GEMM
int zg_gemm_bf16_nt(const uint16_t* A, const uint16_t* B, const float* bias_or_null, void* C, size_t M, size_t N,
                    size_t K, int gelu, int out_bf16) {
    ZG_TRY(require_init());
    ZG_REQUIRE(A && B && C, ZG_ERR_ARG, "gemm_bf16_nt: null argument");
    ZG_REQUIRE(is_device_ptr(A) && is_device_ptr(B) && is_device_ptr(C) && (!bias_or_null || is_device_ptr(bias_or_null)),
               ZG_ERR_ARG, "gemm_bf16_nt: operands must be device pointers");
    ZG_REQUIRE(M < (1u << 30) && N < (1u << 30) && K < (1u << 30), ZG_ERR_SHAPE, "gemm_bf16_nt: dimension too large");
    return launch_gemm_bf16_nt(A, B, bias_or_null, C, (int)M, (int)N, (int)K, (int)N, gelu != 0, out_bf16 != 0,
                               ctx().stream);
}

int zg_debug_prefill_linear(const uint16_t* A, const uint16_t* W, const float* bias, void* C, size_t M, size_t N, size_t K, int epilogue,
                            int force_kernel, int slices, float* ws, size_t ws_floats) {
    ZG_TRY(require_init());
    ZG_REQUIRE(A && W && C && is_device_ptr(A) && is_device_ptr(W) && is_device_ptr(C) && (!bias || is_device_ptr(bias)) && (!ws || is_device_ptr(ws)),
               ZG_ERR_ARG, "debug_prefill_linear: device pointers");
    ZG_REQUIRE(M >= 1 && M < (1u << 30) && N >= 64 && N < (1u << 30) && K >= 64 && K < (1u << 30) && epilogue >= 0 && epilogue <= 2 && force_kernel >= 0 &&
                   force_kernel <= 2 && slices >= 0,
               ZG_ERR_ARG, "debug_prefill_linear: arguments");
    const int epi = epilogue == 0 ? PF_F32 : epilogue == 1 ? PF_RESID : PF_GELU_SPLIT;
    const PrefillForce force{force_kernel, slices};
    return launch_prefill_gemm(A, W, bias, C, (int)M, (int)N, (int)K, epi == PF_GELU_SPLIT ? 0 : (int)N, epi, ws, ws_floats, nullptr, ctx().stream, nullptr,
                               kSplit, &force);
}

int zg_debug_attn_prefill(const float* qkv, uint16_t* out, size_t batch, size_t n_tokens, size_t n_embed, size_t n_heads, const float* k_cache,
                          const float* v_cache, size_t ctx_len, float* ws, size_t ws_floats, int key_tiles) {
    ZG_TRY(require_init());
    ZG_REQUIRE(qkv && out && is_device_ptr(qkv) && is_device_ptr(out) && (!k_cache || (v_cache && is_device_ptr(k_cache) && is_device_ptr(v_cache))) &&
                   (!ws || is_device_ptr(ws)),
               ZG_ERR_ARG, "debug_attn_prefill: device pointers");
    ZG_REQUIRE(batch >= 1 && n_tokens >= 1 && n_heads >= 1 && n_embed == 64 * n_heads && batch * n_tokens < (1u << 24) && n_embed < (1u << 16) && (!k_cache || ctx_len >= n_tokens) &&
                   key_tiles >= 0 && key_tiles <= 255,
               ZG_ERR_ARG, "debug_attn_prefill: arguments");
    return launch_attn_prefill(qkv, out, (int)batch, 0, (int)n_tokens, (int)n_embed, (int)n_heads, ws, ws_floats, PrefillKv{k_cache, v_cache, 0, 0, (int)ctx_len},
                               ctx().stream, key_tiles);
}

int zg_debug_attn_prefill_at(const float* qkv, uint16_t* out, size_t batch, size_t past_len, size_t n_tokens, size_t n_embed, size_t n_heads,
                             const void* k_cache, const void* v_cache, int kv_mode, size_t ctx_len, float* ws, size_t ws_floats, int key_tiles) {
    ZG_TRY(require_init());
    ZG_REQUIRE(qkv && out && k_cache && v_cache && is_device_ptr(qkv) && is_device_ptr(out) && is_device_ptr(k_cache) && is_device_ptr(v_cache) &&
                   (!ws || is_device_ptr(ws)),
               ZG_ERR_ARG, "debug_attn_prefill_at: device pointers");
    ZG_REQUIRE(batch >= 1 && n_tokens >= 1 && n_heads >= 1 && n_embed == 64 * n_heads && batch * n_tokens < (1u << 24) && n_embed < (1u << 16) &&
                   ctx_len < (1u << 22) && past_len + n_tokens <= ctx_len && kv_mode >= 0 && kv_mode <= 2 && key_tiles >= 0 && key_tiles <= 255,
               ZG_ERR_ARG, "debug_attn_prefill_at: arguments");
    return launch_attn_prefill(qkv, out, (int)batch, (int)past_len, (int)n_tokens, (int)n_embed, (int)n_heads, ws, ws_floats,
                               PrefillKv{k_cache, v_cache, kv_mode, batch * ctx_len * n_embed * 2, (int)ctx_len}, ctx().stream, key_tiles);
}

int zg_debug_prefill_route(int force_kernel, int slices) {
    ZG_REQUIRE(force_kernel >= 0 && (force_kernel <= 2 || force_kernel >= 16) && slices >= 0, ZG_ERR_ARG, "debug_prefill_route: arguments");
    prefill_force_route(force_kernel, slices);
    return ZG_OK;
}

unsigned long long zg_debug_gemm_launches(void) { return gemm_mfma_launch_count(); }
int zg_debug_gemm_stamps(unsigned long long* out, size_t n_words) { return gemm_debug_stamps(out, n_words); }
// The op tier's completion word in front of its wrap / what became of it (tests; include/zgpt2.h).  The library stream is drained
// first: no call is in flight whose number the word still has to take.
int zg_debug_ops_set_done_seq(unsigned seq) {
    ZG_TRY(require_init());
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    c.done_seq = seq;
    return ZG_OK;
}
int zg_debug_ops_done_state(unsigned long long* out, size_t n_out) {
    ZG_TRY(require_init());
    ZG_REQUIRE(out && n_out >= 3, ZG_ERR_ARG, "ops_done_state: need 3 words");
    Ctx& c = ctx();
    ZG_HIP(hipStreamSynchronize(c.stream));
    out[0] = c.done_seq;
    out[1] = c.done_flag ? __atomic_load_n(c.done_flag, __ATOMIC_ACQUIRE) : 0u;
    out[2] = c.done_missed;
    return ZG_OK;
}
int zg_debug_last_kernel(char* out, size_t n) {
    if (!out || n == 0) return ZG_ERR_ARG;
    snprintf(out, n, "%s", zg::g_kernel);
    return ZG_OK;
}

// Plans a described decode-regime Linear (gemv_plan) without a GPU or zg_init.  Only null / non-null of the operands matters to
// the planner, so present ones are any non-null address; nothing is dereferenced.
int zg_debug_gemv_plan(int M, int N, int K, int prologue, int epilogue, int weight_type, unsigned operands, int sk_tiles, int t_hi, int* out,
                       size_t n_out) {
    ZG_REQUIRE(out != nullptr && n_out >= ZG_GEMV_PLAN_INTS, ZG_ERR_ARG, "debug_gemv_plan: %d ints of output", ZG_GEMV_PLAN_INTS);
    static float some[2];
    const bool ragged = (operands & ZG_PLAN_RAGGED_STRIDES) != 0;  // row strides wider than the rows
    GemvArgs a{};
    a.M = M;
    a.N = N;
    a.K = K;
    a.prologue = prologue;
    a.epilogue = epilogue;
    a.head_dim = 64;
    a.t_hi = t_hi;
    a.x_stride = K + (ragged ? 8 : 0);
    a.y_stride = a.resid_stride = N + (ragged ? 8 : 0);
    if (operands & ZG_PLAN_LN_FOLDED) a.ln_c2 = a.ln_c3 = some;
    if (operands & ZG_PLAN_PLANES_IN) a.pl_in = reinterpret_cast<const bf16_t*>(some);
    if (operands & ZG_PLAN_STATS_IN) a.st_in = some;
    if (operands & ZG_PLAN_SPLIT_K) {
        a.sk_ws = some;
        a.sk_cnt = reinterpret_cast<int*>(some);
        a.sk_tiles = sk_tiles;
    }
    const GemvPlan p = gemv_plan(a, weight_type);
    const int v[ZG_GEMV_PLAN_INTS] = {p.route, p.grid, p.kslices, p.block, p.lds, p.mt, p.lpr, p.cpl, p.ks, p.nw, p.line, p.gpl, p.alias, p.pairs,
                                      p.steps, p.rows_per_wave, p.waves_per_wg, p.row_group, p.rows_per_wg, p.pf_tiles, p.supported,
                                      p.can_take_planes, p.can_write_planes, p.pl4_with_planes};
    memcpy(out, v, sizeof(v));
    return ZG_OK;
}

// Plans a described whole-prompt Linear (prefill_gemm_plan) without a GPU or zg_init.  Presence flags stand in for the operands;
// nothing is dereferenced.  The process-wide pin of zg_debug_prefill_route is not read: the force is this call's.
int zg_debug_prefill_plan(int M, int N, int K, int ldc, int epilogue, int nsplit, size_t ws_floats, unsigned operands, size_t sk_ws_bytes,
                          unsigned sk_flags_words, int force_kernel, int force_slices, int* out, size_t n_out) {
    ZG_REQUIRE(out != nullptr && n_out >= ZG_PREFILL_PLAN_INTS, ZG_ERR_ARG, "debug_prefill_plan: %d ints of output", ZG_PREFILL_PLAN_INTS);
    PrefillGemmShape sh{M, N, K, ldc, epilogue, nsplit, ws_floats, (operands & ZG_PFPLAN_WS) != 0, (operands & ZG_PFPLAN_LN) != 0,
                        (operands & ZG_PFPLAN_QKV) ? N / 3 : 0, (operands & ZG_PFPLAN_SK_WS) != 0, (operands & ZG_PFPLAN_SK_FLAGS) != 0, sk_ws_bytes,
                        sk_flags_words, PrefillForce{force_kernel, force_slices}};
    const PrefillGemmPlan p = prefill_gemm_plan(sh);
    static_assert(ZG_PREFILL_PLAN_INTS == 21, "prefill_plan_ints packs 21");
    prefill_plan_ints(p, out);
    return ZG_OK;
}

int zg_f32_to_bf16(const float* src, uint16_t* dst_device, size_t len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(src && dst_device && is_device_ptr(dst_device), ZG_ERR_ARG, "f32_to_bf16: bad argument");
    Call call;
    CallGuard guard(call);
    const float* s;
    ZG_TRY(call.in(src, len, &s));
    ZG_TRY(launch_f32_to_bf16(s, dst_device, len, call.stream()));
    ZG_TRY(call.finish());
    guard.done = true;
    return ZG_OK;
}

// ------------------------------------------------------------------------------ Embedding
int zg_embedding_forward(size_t emb_dim, const float* weight, size_t weight_len, const size_t* idxs,
                         size_t idxs_len, float* embeddings, size_t embeddings_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(emb_dim > 0 && weight && (idxs || idxs_len == 0) && (embeddings || idxs_len == 0), ZG_ERR_ARG, "Embedding: null argument");
    ZG_REQUIRE(embeddings_len >= idxs_len * emb_dim, ZG_ERR_SHAPE,
               "Embedding: embeddings.len %zu < %zu indices * emb_dim %zu", embeddings_len, idxs_len, emb_dim);
    Call call;
    CallGuard guard(call);
    const float* w;
    const size_t* ix;
    float* out;
    ZG_TRY(call.param(weight, weight_len, &w));
    ZG_TRY(call.in_once(idxs, idxs_len, &ix));
    ZG_TRY(call.out_once(embeddings, idxs_len * emb_dim, &out));
    unsigned* df;
    unsigned ds;
    bool own = false;
    call.reserve(&df, &ds);
    ZG_TRY(launch_embedding(w, emb_dim, ix, idxs_len, weight_len / emb_dim, out, ctx().d_flag, call.stream(), df, ds, &own));
    call.announced(own);
    ZG_TRY(call.finish());
    guard.done = true;
    if (*static_cast<volatile int*>(ctx().d_flag)) {  // raised by the kernel (pinned host word), read behind the call's drain
        *ctx().d_flag = 0;
        set_error("embedding: index out of range (>= %zu rows)", weight_len / emb_dim);
        return ZG_ERR_SHAPE;  // (the rows of valid indices were written, like the reference up to its bounds panic)
    }
    return ZG_OK;
}

// ------------------------------------------------------------------------------ LayerNorm
int zg_layernorm_forward(size_t n_features, const float* weight, const float* bias, float eps,
                         float* inputs, size_t inputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(n_features > 0 && weight && bias && (inputs || inputs_len == 0), ZG_ERR_ARG, "LayerNorm: null argument");
    const size_t rows = inputs_len / n_features;
    ZG_REQUIRE(inputs_len == rows * n_features, ZG_ERR_SHAPE,
               "LayerNorm: inputs.len %zu is not a multiple of n_features %zu", inputs_len, n_features);
    Call call;
    CallGuard guard(call);
    const float *g, *b;
    float* x;
    ZG_TRY(call.param(weight, n_features, &g));
    ZG_TRY(call.param(bias, n_features, &b));
    ZG_TRY(call.inout_once(inputs, inputs_len, &x));
    unsigned* df;
    unsigned ds;
    bool own = false;
    call.reserve(&df, &ds);
    Ctx& c = ctx();
    const size_t bytes = inputs_len * sizeof(float);
    const bool twin = static_cast<void*>(x) != static_cast<void*>(inputs) && bytes <= c.shadow_cap;  // a host buffer: keep a device twin of the result
    c.shadow_ptr = nullptr;
    ZG_TRY(launch_layernorm(x, (int)rows, (int)n_features, g, b, eps, call.stream(), df, ds, &own, twin ? c.shadow_dev : nullptr));
    call.announced(own);
    ZG_TRY(call.finish());
    guard.done = true;
    if (twin) {
        memcpy(c.shadow_host, inputs, bytes);
        c.shadow_ptr = inputs;
        c.shadow_bytes = bytes;
    }
    return ZG_OK;
}

// ------------------------------------------------------------------------------ gelu / softmax
int zg_gelu(float* inputs, size_t inputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(inputs || inputs_len == 0, ZG_ERR_ARG, "gelu: null argument");
    Call call;
    CallGuard guard(call);
    float* x;
    ZG_TRY(call.inout_once(inputs, inputs_len, &x));
    unsigned* df;
    unsigned ds;
    bool own = false;
    call.reserve(&df, &ds);
    Ctx& c = ctx();
    const size_t bytes = inputs_len * sizeof(float);
    const bool twin = static_cast<void*>(x) != static_cast<void*>(inputs) && bytes <= c.shadow_cap;
    c.shadow_ptr = nullptr;
    ZG_TRY(launch_gelu(x, inputs_len, call.stream(), df, ds, &own, twin ? c.shadow_dev : nullptr));
    call.announced(own);
    ZG_TRY(call.finish());
    guard.done = true;
    if (twin) {
        memcpy(c.shadow_host, inputs, bytes);
        c.shadow_ptr = inputs;
        c.shadow_bytes = bytes;
    }
    return ZG_OK;
}

int zg_softmax(float* inputs, size_t inputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(inputs || inputs_len == 0, ZG_ERR_ARG, "softmax: null argument");
    Call call;
    CallGuard guard(call);
    float* x;
    ZG_TRY(call.inout_once(inputs, inputs_len, &x));
    unsigned* df;
    unsigned ds;
    bool own = false;
    call.reserve(&df, &ds);
    ZG_TRY(launch_softmax(x, inputs_len, call.stream(), df, ds, &own));
    call.announced(own);
    ZG_TRY(call.finish());
    guard.done = true;
    return ZG_OK;
}

// ------------------------------------------------------------------------------ split / transpose
int zg_split_qkv(size_t n_embed, size_t seq_len, const float* inputs, size_t inputs_len,
                 size_t split_idx, float* outputs, size_t outputs_len) {
    ZG_TRY(require_init());
    ZG_REQUIRE(n_embed > 0 && seq_len > 0 && split_idx < 3, ZG_ERR_ARG, "split_qkv: bad argument");
    const size_t batch = inputs_len / (seq_len * 3 * n_embed);  // ops.zig:185
    const size_t rows = batch * seq_len;
    ZG_REQUIRE(rows == 0 || (inputs && outputs), ZG_ERR_ARG, "split_qkv: null argument");
    ZG_REQUIRE(outputs_len >= rows * n_embed, ZG_ERR_SHAPE, "split_qkv: outputs.len %zu < %zu", outputs_len,
               rows * n_embed);
    Call call;
    CallGuard guard(call);
    const float* in;
    float* out;
    ZG_TRY(call.in_once(inputs, inputs_len, &in));
    ZG_TRY(call.out_once(outputs, rows * n_embed, &out));
    ZG_TRY(launch_split_qkv(in, rows, n_embed, split_idx, out, call.stream()));
    ZG_TRY(call.finish());
    guard.done = true;
    return ZG_OK;
}

int zg_transpose(size_t seq_len, size_t n_heads, size_t head_dim, const float* inputs,
                 size_t inputs_len, float* outputs, size_t outputs_len) {
    ZG_TRY(require_init());
    const size_t per = seq_len * n_heads * head_dim;
    ZG_REQUIRE(per > 0, ZG_ERR_ARG, "transpose: empty shape");
    const size_t batch = inputs_len / per;  // ops.zig:203
    ZG_REQUIRE(batch == 0 || (inputs && outputs), ZG_ERR_ARG, "transpose: null argument");
    ZG_REQUIRE(outputs_len >= batch * per, ZG_ERR_SHAPE, "transpose: outputs.len %zu < %zu", outputs_len, batch * per);
    ZG_REQUIRE(n_heads <= 65535 && batch <= 65535, ZG_ERR_UNSUPPORTED, "transpose: n_heads/batch > 65535");
    Call call;
    CallGuard guard(call);
    const float* in;
    float* out;
    ZG_TRY(call.in_once(inputs, inputs_len, &in));
    ZG_TRY(call.out_once(outputs, batch * per, &out));
    ZG_TRY(launch_transpose(in, batch, seq_len, n_heads, head_dim, out, call.stream()));
    ZG_TRY(call.finish());
    guard.done = true;
    return ZG_OK;
}

// ------------------------------------------------------------------------------ sdpa
int zg_scaled_dot_product_attention(const float* q, size_t q_len, const float* k, size_t k_len,
                                    const float* v, size_t v_len, size_t n_heads, size_t seq_len,
                                    size_t head_dim, float* outputs, size_t outputs_len, float* _attn,
                                    size_t _attn_len) {
    ZG_TRY(require_init());
    (void)_attn;
    ZG_REQUIRE(n_heads > 0 && seq_len > 0 && head_dim > 0, ZG_ERR_ARG, "sdpa: empty shape");
    ZG_REQUIRE(head_dim <= 2048, ZG_ERR_UNSUPPORTED, "sdpa: head_dim %zu beyond 2048", head_dim);
    const size_t batch = k_len / (n_heads * seq_len * head_dim);  // ops.zig:259
    ZG_REQUIRE(batch == 0 || (q && k && v && outputs), ZG_ERR_ARG, "sdpa: null argument");
    ZG_REQUIRE(v_len >= k_len && q_len >= batch * n_heads * head_dim && outputs_len >= batch * n_heads * head_dim &&
                   _attn_len >= seq_len,
               ZG_ERR_SHAPE, "sdpa: slice lengths inconsistent with batch %zu", batch);
    Call call;
    CallGuard guard(call);
    const float *dq, *dk, *dv;
    float* out;
    ZG_TRY(call.in(q, batch * n_heads * head_dim, &dq));
    ZG_TRY(call.in(k, k_len, &dk));
    ZG_TRY(call.in(v, k_len, &dv));
    ZG_TRY(call.out_once(outputs, batch * n_heads * head_dim, &out));
    ZG_TRY(attn_core(dq, dk, dv, (long)(n_heads * seq_len * head_dim), (long)(seq_len * head_dim), (long)head_dim,
                     batch, n_heads, seq_len, out, call.stream(), head_dim));
    ZG_TRY(call.finish());
    guard.done = true;
    return ZG_OK;
}

// ------------------------------------------------------------------------------ CausalSelfAttention
int zg_attn_forward(size_t n_heads, size_t n_embed, const float* c_attn_weight, const float* c_attn_bias,
                    const float* c_proj_weight, const float* c_proj_bias, size_t seq_len,
                    const float* inputs, size_t inputs_len, float* k_cache, size_t k_cache_len,
                    float* v_cache, size_t v_cache_len, float* outputs, size_t outputs_len, float* _qkv,
                    size_t _qkv_len, float* _q, size_t _q_len, float* _k, size_t _k_len, float* _v,
                    size_t _v_len, float* _attn, size_t _attn_len) {
    ZG_TRY(require_init());
    (void)_k;
    (void)_v;
    (void)_attn;
    const size_t E = n_embed;
    ZG_REQUIRE(n_heads > 0 && E > 0 && seq_len > 0, ZG_ERR_ARG, "attn: empty shape");
    ZG_REQUIRE(E % n_heads == 0, ZG_ERR_SHAPE, "attn: n_embed %zu is not a multiple of n_heads %zu", E, n_heads);
    const size_t hd = E / n_heads;  // 64 for every GPT-2 configuration; anything else takes the op tier's general attention kernel
    ZG_REQUIRE(inputs_len == E, ZG_ERR_SHAPE, "attn: batch must be 1 (inputs.len %zu != n_embed %zu; ops.zig:126-128)",
               inputs_len, E);
    ZG_REQUIRE(k_cache_len >= seq_len * E && v_cache_len >= seq_len * E && outputs_len >= E &&
                   _qkv_len >= 3 * E && _q_len >= E && _k_len >= seq_len * E && _v_len >= seq_len * E &&
                   _attn_len >= seq_len,
               ZG_ERR_SHAPE, "attn: a slice is shorter than seq_len %zu * n_embed %zu requires", seq_len, E);
    ZG_REQUIRE(c_attn_weight && c_attn_bias && c_proj_weight && c_proj_bias && inputs && k_cache && v_cache && outputs && _qkv && _q, ZG_ERR_ARG,
               "attn: null argument");
    ZG_REQUIRE(hd <= 2048, ZG_ERR_UNSUPPORTED, "attn: head_dim %zu beyond 2048", hd);
    Call call;
    CallGuard guard(call);
    hipStream_t s = call.stream();
    Ctx& c = ctx();
    const float *caw, *cab, *cpw, *cpb, *x;
    float *kc = nullptr, *vc = nullptr, *out, *qkv, *q;
    ZG_TRY(call.param(c_attn_weight, 3 * E * E, &caw));
    ZG_TRY(call.param(c_attn_bias, 3 * E, &cab));
    ZG_TRY(call.param(c_proj_weight, E * E, &cpw));
    ZG_TRY(call.param(c_proj_bias, E, &cpb));
    ZG_TRY(call.in(inputs, E, &x));
    // The caller owns the caches and appends one row per call (ops.zig:152,157); what it can observe afterwards is row T-1.
    // Host caches are mirrored on the device, keyed by their address: when this call continues the sequence the mirror holds
    // (same pointer, same width, seq_len = rows held + 1) nothing goes up and only the new row comes back; anything else
    // — a first sight, a restart, a jump — uploads rows 0 .. T-2 again.  A caller that EDITS earlier rows in place between two
    // consecutive positions must drop the mirror (zg_unregister_tensor(cache)).  No room in the pool: the whole cache is staged.
    KvMirror* mir[2] = {nullptr, nullptr};
    float* host_cache[2] = {k_cache, v_cache};
    float** dev_cache[2] = {&kc, &vc};
    {   // The pool is a bump allocator and mirrors of caches the caller has long freed stay in it.  When this call's caches would
        // not fit what is left, every mirror is dropped and the pool starts over (the live caches upload once more at their next
        // call) — before any pointer into the map is taken.
        size_t need_bytes = 0;
        for (int i = 0; i < 2; ++i) {
            if (is_device_ptr(host_cache[i])) continue;
            auto it = c.kv_mirrors.find(host_cache[i]);
            if (it == c.kv_mirrors.end() || it->second.cap_floats < seq_len * E) need_bytes += std::max(seq_len * E * 2, (size_t)1024 * E) * sizeof(float) + 256;
        }
        if (need_bytes > 0 && c.kv_pool_off > 0 && c.kv_pool_off + need_bytes > c.kv_pool_cap && need_bytes <= c.kv_pool_cap) {
            c.kv_mirrors.clear();
            c.kv_pool_off = 0;
        }
    }
    for (int i = 0; i < 2; ++i) {
        if (is_device_ptr(host_cache[i])) {
            *dev_cache[i] = host_cache[i];
            continue;
        }
        KvMirror* m = nullptr;
        auto it = c.kv_mirrors.find(host_cache[i]);
        if (it != c.kv_mirrors.end()) m = &it->second;
        const size_t need = seq_len * E;
        if (m == nullptr || m->cap_floats < need) {  // a slot for this cache: the reference's context (1024 rows) or twice what is needed
            const size_t cap = std::max(need * 2, (size_t)1024 * E);
            const size_t off = (c.kv_pool_off + 255) & ~(size_t)255;
            if (c.kv_pool != nullptr && off + cap * sizeof(float) <= c.kv_pool_cap) {
                KvMirror fresh;
                fresh.dev = reinterpret_cast<float*>(c.kv_pool + off);
                fresh.cap_floats = cap;
                fresh.n_embed = E;
                fresh.rows = 0;
                c.kv_pool_off = off + cap * sizeof(float);
                m = &(c.kv_mirrors[host_cache[i]] = fresh);  // (an outgrown slot stays behind until zg_unregister_all)
            } else {
                m = nullptr;
                c.kv_mirrors.erase(host_cache[i]);
            }
        }
        if (m == nullptr) {  // pool exhausted: rows 0..T-2 go up, row T-1 comes back, every call
            ZG_TRY(call.inout(host_cache[i], seq_len * E, dev_cache[i]));
            continue;
        }
        if (m->n_embed != E || m->rows + 1 != seq_len) {
            if (seq_len > 1) ZG_HIP(hipMemcpyAsync(m->dev, host_cache[i], (seq_len - 1) * E * sizeof(float), hipMemcpyHostToDevice, s));
            m->n_embed = E;
        }
        m->rows = 0;  // (valid again once this call has succeeded)
        mir[i] = m;
        *dev_cache[i] = m->dev;
    }
    ZG_TRY(call.out_once(outputs, E, &out));  // stored once by c_proj
    ZG_TRY(call.out(_qkv, 3 * E, &qkv));      // read back by the append and the attention: device memory
    ZG_TRY(call.out(_q, E, &q));
    // c_attn (ops.zig:143)
    ZG_TRY(linear_device(E, 3 * E, caw, cab, x, 1, qkv, s));
    // cache append (ops.zig:151-152, :156-157): into the device cache, and — for mirrored host caches — row T-1 back to the caller
    ZG_TRY(launch_copy2_f32(qkv + E, kc + (seq_len - 1) * E, qkv + 2 * E, vc + (seq_len - 1) * E, E, s));
    if (mir[0]) ZG_TRY(call.also_out(k_cache + (seq_len - 1) * E, qkv + E, E * sizeof(float)));
    if (mir[1]) ZG_TRY(call.also_out(v_cache + (seq_len - 1) * E, qkv + 2 * E, E * sizeof(float)));
    // attention straight over the [T, H, hd] cache (replaces transposes + sdpa, ops.zig:153-171);
    // the merged heads land in _q like the reference's "untranspose" (ops.zig:171)
    ZG_TRY(attn_core(qkv, kc, vc, 0, (long)hd, (long)E, 1, n_heads, seq_len, q, s, hd));
    // c_proj (ops.zig:172)
    ZG_TRY(linear_device(E, E, cpw, cpb, q, 1, out, s));
    ZG_TRY(call.finish());
    guard.done = true;
    for (KvMirror* m : mir)
        if (m) m->rows = seq_len;
    return ZG_OK;
}

}  // extern "C"
