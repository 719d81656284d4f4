// elementwise.hip — the small ops of reference src/ops.zig as standalone HIP kernels (op tier), the copies and the format
// conversions (bf16, B24, bf16 planes) of both tiers.  All are HBM/latency bound; loads are 16 B per lane where the layout
// allows.  (The head of a decode step and the sampler stages: sample.hip.)
#include <algorithm>

#include "zg_kernels.h"

namespace zg {

namespace {

__device__ __forceinline__ float block_allsum(float v, float* s_red) {
    v = wave_allsum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    float t = 0.0f;
    for (int w = 0; w < nw; ++w) t += s_red[w];
    return t;
}

__device__ __forceinline__ float block_allmax(float v, float* s_red) {
    v = wave_allmax(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    float t = s_red[0];
    for (int w = 1; w < nw; ++w) t = fmaxf(t, s_red[w]);
    return t;
}

// A single-workgroup kernel of the op tier may announce its own completion: every lane fences its stores to the system, then
// behind a workgroup barrier (waves that have left no longer count) one lane stores the call's sequence number into the pinned
// completion word the host polls (Call::finish) — the separate one-thread launch (2.7 us on the device) is then skipped.
struct DoneWord {
    unsigned* flag;  // nullptr: not asked
    unsigned seq;
};
__device__ inline void announce_done(const DoneWord d) {
    if (d.flag == nullptr) return;
    // every wave waits until its own stores have been acknowledged by the L2 (the workgroup's waves share one XCD's L2), then the
    // barrier, then ONE lane releases to system scope — the L2-wide write-back covers all waves' stores — and stores the word.
    // (A system-scope fence in every lane was measured: +1.3 us on LayerNorm, +4.8 us on gelu — one L2 write-back per wave.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(d.flag, d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// LayerNorm.forward (src/ops.zig:82-104): one wave per row, in place.  Rows of up to 64 x 32 elements are held in registers
// between the statistics and the normalisation: every element is read once and written once (the op tier hands small host
// buffers over in place, across PCIe).
__global__ __launch_bounds__(256) void layernorm_kernel(float* x, int rows, int n, const float* g,
                                                        const float* b, float eps, DoneWord done, float* shadow) {
    // shadow (op tier, may be null): a device-memory twin of the result — x itself may be pinned host memory the NEXT op's
    // kernels should not read across PCIe (zg_runtime.h Shadow: the output of one op is the input of the next Linear in src/main.zig)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row < rows) {
        float* r = x + (size_t)row * n;
        float s1 = 0.0f, s2 = 0.0f;
        if (n <= 64 * 32) {
            float v[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int i = lane + 64 * j;
                v[j] = i < n ? r[i] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                s1 += v[j];
                s2 = fmaf(v[j], v[j], s2);
            }
            s1 = wave_allsum(s1);
            s2 = wave_allsum(s2);
            const float mean = s1 / (float)n;
            const float std_ = sqrtf(s2 / (float)n - mean * mean + eps);
#pragma unroll
            for (int j = 0; j < 32; ++j) {
                const int i = lane + 64 * j;
                if (i < n) {
                    const float y = (v[j] - mean) / std_ * g[i] + b[i];
                    r[i] = y;
                    if (shadow) shadow[(size_t)row * n + i] = y;
                }
            }
        } else {
            for (int i = lane; i < n; i += 64) {
                const float v = r[i];
                s1 += v;
                s2 = fmaf(v, v, s2);
            }
            s1 = wave_allsum(s1);
            s2 = wave_allsum(s2);
            const float mean = s1 / (float)n;
            const float std_ = sqrtf(s2 / (float)n - mean * mean + eps);
            for (int i = lane; i < n; i += 64) {
                const float y = (r[i] - mean) / std_ * g[i] + b[i];
                r[i] = y;
                if (shadow) shadow[(size_t)row * n + i] = y;
            }
        }
    }
    announce_done(done);  // (asked for only when the grid is one workgroup)
}

// gelu (src/ops.zig:221-228), in place.
__global__ __launch_bounds__(1024) void gelu_kernel(float* x, size_t n, DoneWord done, float* shadow) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t n4 = n / 4;
    f32x4* x4 = reinterpret_cast<f32x4*>(x);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 v = x4[i];
        v.x = gelu_ref(v.x); v.y = gelu_ref(v.y); v.z = gelu_ref(v.z); v.w = gelu_ref(v.w);
        x4[i] = v;
        if (shadow) reinterpret_cast<f32x4*>(shadow)[i] = v;
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float y = gelu_ref(x[i]);
        x[i] = y;
        if (shadow) shadow[i] = y;
    }
    announce_done(done);  // (asked for only when the grid is one workgroup)
}

// softmax (src/ops.zig:231-241): the whole slice is one vector; single workgroup, in place.  Up to 1024 x 64 elements (the
// logits of every GPT-2 vocabulary, src/main.zig:203) stay in registers across the three passes: read once, written once.
__global__ __launch_bounds__(1024) void softmax_kernel(float* x, size_t n, DoneWord done) {
    __shared__ float s_red[16];
    if (n <= (size_t)1024 * 64) {
        float v[64];
        float mx = -3.0e38f;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const size_t i = threadIdx.x + (size_t)1024 * j;
            v[j] = i < n ? x[i] : -3.0e38f;
            mx = fmaxf(mx, v[j]);
        }
        mx = block_allmax(mx, s_red);
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const size_t i = threadIdx.x + (size_t)1024 * j;
            v[j] = i < n ? __expf(v[j] - mx) : 0.0f;
            sum += v[j];
        }
        sum = block_allsum(sum, s_red);
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            const size_t i = threadIdx.x + (size_t)1024 * j;
            if (i < n) x[i] = v[j] / sum;
        }
        announce_done(done);
        return;
    }
    float mx = -3.0e38f;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) mx = fmaxf(mx, x[i]);
    mx = block_allmax(mx, s_red);
    float sum = 0.0f;
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float e = __expf(x[i] - mx);
        x[i] = e;
        sum += e;
    }
    sum = block_allsum(sum, s_red);
    for (size_t i = threadIdx.x; i < n; i += blockDim.x) x[i] = x[i] / sum;
    announce_done(done);
}

// Embedding.forward (src/ops.zig:59-67): out[i] = weight[idx[i]].
__global__ __launch_bounds__(256) void embedding_kernel(const float* w, size_t emb_dim, const size_t* idx,
                                                        size_t n_rows, float* out, int* oob, DoneWord done) {
    const size_t i = blockIdx.x;
    const size_t id = idx[i];
    if (id >= n_rows) {
        if (threadIdx.x == 0) *oob = 1;
    } else {
        for (size_t e = threadIdx.x; e < emb_dim; e += blockDim.x) out[i * emb_dim + e] = w[id * emb_dim + e];
    }
    announce_done(done);  // (asked for only when the grid is one workgroup)
}

// split_qkv (src/ops.zig:177-196): rows x [3E] -> rows x [E].
__global__ __launch_bounds__(256) void split_qkv_kernel(const float* in, size_t n_embed, size_t split_idx,
                                                        float* out) {
    const size_t r = blockIdx.x;
    for (size_t e = threadIdx.x; e < n_embed; e += blockDim.x)
        out[r * n_embed + e] = in[r * 3 * n_embed + split_idx * n_embed + e];
}

// transpose (src/ops.zig:199-216): (b,t,n,h) -> (b,n,t,h); one workgroup per (b,n,t) run of h.
__global__ __launch_bounds__(64) void transpose_kernel(const float* in, size_t t, size_t n, size_t h, float* out) {
    const size_t s = blockIdx.x, hh = blockIdx.y, b = blockIdx.z;
    const float* src = in + b * t * n * h + s * n * h + hh * h;
    float* dst = out + b * t * n * h + hh * t * h + s * h;
    for (size_t d = threadIdx.x; d < h; d += blockDim.x) dst[d] = src[d];
}

__global__ __launch_bounds__(256) void copy_kernel(const float* in, float* out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i];
}

__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* in, bf16_t* out, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = f32_to_bf16_rne(in[i]);
}

// fp32 [rows][K] -> bf16 planes [rows][3K] = [hi | mid | lo] with hi + mid + lo == x exactly (8 + 8 + 8 mantissa bits):
// the operand format of launch_gemm_planes.  One thread per 4 consecutive elements (16-B load, three 8-B stores).
__global__ __launch_bounds__(256) void split3_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, size_t rows, int K) {
    const size_t quads = rows * (size_t)(K / 4), stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += stride) {
        const size_t r = i / (K / 4), k = (i % (K / 4)) * 4;
        store_split3x4(out + r * (size_t)(3 * K) + k, (size_t)K, *reinterpret_cast<const f32x4*>(in + r * K + k));
    }
}

// fp32 [rows][K] -> B24 rows: one thread per 8 elements, a 16-B store of upper halves and an 8-B store of low bytes
__global__ __launch_bounds__(256) void f32_to_b24_kernel(const float* __restrict__ in, size_t rows, int K, char* __restrict__ out) {
    const size_t per_row = (size_t)(K / 8), n = rows * per_row;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / per_row, k = (i % per_row) * 8;
        const f32x4 a = *reinterpret_cast<const f32x4*>(in + r * K + k);
        const f32x4 b = *reinterpret_cast<const f32x4*>(in + r * K + k + 4);
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = b24_round(v[j]);  // 24 bits, right-aligned: upper half = q >> 8, low byte = q & 0xff
        char* o = out + r * (size_t)(3 * K);
        *reinterpret_cast<u32x4*>(o + 2 * k) = u32x4{(q[0] >> 8) | ((q[1] >> 8) << 16), (q[2] >> 8) | ((q[3] >> 8) << 16),
                                                     (q[4] >> 8) | ((q[5] >> 8) << 16), (q[6] >> 8) | ((q[7] >> 8) << 16)};
        *reinterpret_cast<u32x2*>(o + 2 * (size_t)K + k) =
            u32x2{(q[0] & 0xffu) | (q[1] & 0xffu) << 8 | (q[2] & 0xffu) << 16 | (q[3] & 0xffu) << 24,
                  (q[4] & 0xffu) | (q[5] & 0xffu) << 8 | (q[6] & 0xffu) << 16 | (q[7] & 0xffu) << 24};
    }
}

// B24 [rows][K] -> plane-major [3][rows K]: split3_kernel's arithmetic on the values the matrix holds (the whole-prompt GEMMs'
// weight operand; its planes are then bit for bit those of an fp32 matrix holding the same values)
__global__ __launch_bounds__(256) void b24_split3_kernel(const char* __restrict__ in, size_t rows, int K, bf16_t* __restrict__ out) {
    const size_t per_row = (size_t)(K / 4), n = rows * per_row, total = rows * (size_t)K;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / per_row, k = (i % per_row) * 4;
        store_split3x4(out + r * K + k, total, load_b24x4(in, r, K, (int)k));
    }
}

// The B operand of the scoring lm_head on fp32 / B24 handles: the stored values of wte [V][K] split exactly into bf16 planes,
// plane-major [3][V64][K] as the whole-prompt GEMMs read weight planes, rows V .. V64 - 1 zero.
__global__ __launch_bounds__(256) void wte_planes_kernel(const void* __restrict__ wte, int weight_type, size_t V, size_t V64, int K, bf16_t* __restrict__ out) {
    const size_t per_row = (size_t)(K / 4), n = V64 * per_row, plane = V64 * (size_t)K;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / per_row, k = (i % per_row) * 4;
        f32x4 v{0.0f, 0.0f, 0.0f, 0.0f};
        if (r < V) v = weight_type == WT_B24 ? load_b24x4(wte, r, K, (int)k) : *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(wte) + r * K + k);
        store_split3x4(out + r * K + k, plane, v);
    }
}

inline int grid_for(size_t n, int block = 256, int cap = 2048) {
    size_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    return (int)(g > (size_t)cap ? cap : g);
}

}  // namespace

// done offers a word (done->flag != nullptr): the caller would like the kernel to announce its own completion; done->taken tells
// whether this launch does (a one-workgroup grid), otherwise the caller's one-thread launch follows as usual.
static bool offered(const DoneSlot* done) { return done != nullptr && done->flag != nullptr; }
static DoneWord word_of(const DoneSlot* done, bool own) { return DoneWord{own ? done->flag : nullptr, done ? done->seq : 0u}; }

int launch_layernorm(float* x, int rows, int n, const float* g, const float* b, float eps, hipStream_t s, DoneSlot* done, float* shadow) {
    if (rows == 0) return ZG_OK;
    const bool own = offered(done) && rows <= 4;
    hipLaunchKernelGGL(layernorm_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, rows, n, g, b, eps, word_of(done, own), shadow);
    ZG_HIP(hipGetLastError());
    if (done) done->taken = own;
    return ZG_OK;
}

int launch_gelu(float* x, size_t n, hipStream_t s, DoneSlot* done, float* shadow) {
    if (n == 0) return ZG_OK;
    const bool own = offered(done) && n <= 4096;  // one workgroup of 1024 lanes, one vector of four each: a single pass
    hipLaunchKernelGGL(gelu_kernel, dim3(own ? 1 : grid_for(n / 4 + 1)), dim3(own ? 1024 : 256), 0, s, x, n, word_of(done, own), shadow);
    ZG_HIP(hipGetLastError());
    if (done) done->taken = own;
    return ZG_OK;
}

int launch_softmax(float* x, size_t n, hipStream_t s, DoneSlot* done) {
    if (n == 0) return ZG_OK;
    const bool own = offered(done);
    hipLaunchKernelGGL(softmax_kernel, dim3(1), dim3(1024), 0, s, x, n, word_of(done, own));
    ZG_HIP(hipGetLastError());
    if (done) done->taken = own;
    return ZG_OK;
}

// The completion word of an op-tier call: the host polls this pinned word instead of paying hipStreamSynchronize's wake-up
// (tools/microbench/sync_cost.hip: 9.6-11.0 against 12.0-13.3 us per one-kernel call).  In stream order behind the call's
// kernels, whose results the kernel boundary has already released to the system.
__global__ void done_flag_kernel(unsigned* flag, unsigned seq) {
    __threadfence_system();
    __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// The outputs of an op-tier call that live in device memory (read back by later kernels of the call, e.g. _qkv and _q of
// CausalSelfAttention.forward) leave for the pinned arena AND the call's completion is announced in ONE launch: a single
// workgroup copies up to four small segments and then stores the completion word — instead of a DMA plus the one-thread launch.
__global__ __launch_bounds__(1024) void copy_out_done_kernel(CopySegs segs, DoneWord done) {
    for (int k = 0; k < segs.n; ++k) {
        const f32x4* src = reinterpret_cast<const f32x4*>(segs.src[k]);
        f32x4* dst = reinterpret_cast<f32x4*>(segs.dst[k]);
        const unsigned n4 = segs.bytes[k] / 16;
        for (unsigned i = threadIdx.x; i < n4; i += 1024) dst[i] = src[i];
        const unsigned tail = segs.bytes[k] & 15u;  // (multiples of 4 bytes: the op tier's element types are 4 or 8 bytes wide)
        if (threadIdx.x < tail / 4) reinterpret_cast<float*>(segs.dst[k])[n4 * 4 + threadIdx.x] = reinterpret_cast<const float*>(segs.src[k])[n4 * 4 + threadIdx.x];
    }
    announce_done(done);
}
int launch_copy_out_done(const CopySegs& segs, unsigned* flag, unsigned seq, hipStream_t s) {
    hipLaunchKernelGGL(copy_out_done_kernel, dim3(1), dim3(1024), 0, s, segs, DoneWord{flag, seq});
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// two equally long copies in one launch (the k and v rows of a cache append, ops.zig:151-152, :156-157)
__global__ __launch_bounds__(256) void copy2_kernel(const float* a, float* da, const float* b, float* db, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        da[i] = a[i];
        db[i] = b[i];
    }
}
int launch_copy2_f32(const float* a, float* da, const float* b, float* db, size_t n, hipStream_t s) {
    if (n == 0) return ZG_OK;
    hipLaunchKernelGGL(copy2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, da, b, db, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_done_flag(unsigned* flag, unsigned seq, hipStream_t s) {
    hipLaunchKernelGGL(done_flag_kernel, dim3(1), dim3(1), 0, s, flag, seq);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

__global__ void epoch_bump_kernel(unsigned* epoch) { *epoch += 1u; }
int launch_epoch_bump(unsigned* epoch, hipStream_t s) {
    hipLaunchKernelGGL(epoch_bump_kernel, dim3(1), dim3(1), 0, s, epoch);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}
__global__ void epoch_add_kernel(unsigned* epoch, unsigned n) { *epoch += n; }
int launch_epoch_add(unsigned* epoch, unsigned n, hipStream_t s) {
    hipLaunchKernelGGL(epoch_add_kernel, dim3(1), dim3(1), 0, s, epoch, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_embedding(const float* w, size_t emb_dim, const size_t* idx, size_t n_idx, size_t n_rows,
                     float* out, int* d_oob, hipStream_t s, DoneSlot* done) {
    if (n_idx == 0) return ZG_OK;
    // (d_oob is a pinned host word: the caller reads it behind its own drain of the stream)
    const bool own = offered(done) && n_idx == 1;
    hipLaunchKernelGGL(embedding_kernel, dim3((unsigned)n_idx), dim3(256), 0, s, w, emb_dim, idx, n_rows, out, d_oob, word_of(done, own));
    ZG_HIP(hipGetLastError());
    if (done) done->taken = own;
    return ZG_OK;
}

int launch_split_qkv(const float* in, size_t rows, size_t n_embed, size_t split_idx, float* out, hipStream_t s) {
    if (rows == 0) return ZG_OK;
    hipLaunchKernelGGL(split_qkv_kernel, dim3((unsigned)rows), dim3(256), 0, s, in, n_embed, split_idx, out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_transpose(const float* in, size_t batch, size_t t, size_t n, size_t h, float* out, hipStream_t s) {
    if (batch * t * n * h == 0) return ZG_OK;
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)t, (unsigned)n, (unsigned)batch), dim3(64), 0, s, in, t, n, h, out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_copy_f32(const float* in, float* out, size_t n, hipStream_t s) {
    if (n == 0) return ZG_OK;
    hipLaunchKernelGGL(copy_kernel, dim3(grid_for(n)), dim3(256), 0, s, in, out, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_f32_to_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s) {
    if (n == 0) return ZG_OK;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(grid_for(n)), dim3(256), 0, s, in, out, n);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

static __global__ __launch_bounds__(256) void kv_clear_tail_kernel(char* base, size_t cache_stride, size_t plane_off, int row_bytes, int strips, int ctx,
                                                            int from_row) {
    const int strip = blockIdx.x, cache = blockIdx.y;
    char* p = base + (size_t)cache * cache_stride + plane_off + ((size_t)strip * ctx + from_row) * row_bytes;
    const size_t n16 = (size_t)(ctx - from_row) * row_bytes / 16;  // (row_bytes is a multiple of 64)
    for (size_t i = threadIdx.x; i < n16; i += 256) reinterpret_cast<u32x4*>(p)[i] = u32x4{0u, 0u, 0u, 0u};
}

int launch_kv_clear_tail(void* base, int n_caches, size_t cache_stride, size_t plane_off, int row_bytes, int strips, int ctx, int from_row,
                         hipStream_t s) {
    if (from_row >= ctx || n_caches == 0 || strips == 0) return ZG_OK;
    ZG_REQUIRE(row_bytes % 64 == 0 && strips < 65536 * 32 && n_caches < 65536, ZG_ERR_UNSUPPORTED, "kv clear: %d-byte rows, %d strips", row_bytes, strips);
    hipLaunchKernelGGL(kv_clear_tail_kernel, dim3(strips, n_caches), dim3(256), 0, s, reinterpret_cast<char*>(base), cache_stride, plane_off, row_bytes,
                       strips, ctx, from_row);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

// One workgroup per (64-position tile, head, cache x destination row): at most 16 KB of one head's strip, as 16-byte loads that are
// all issued before the first store.  The row's source and the cached length are clamped before they become addresses; a
// row that is its own source leaves on a uniform branch before any load, and so does a tile at or behind the cached length.
static __global__ __launch_bounds__(256) void kv_fork_kernel(KvForkArgs a) {
    const int tile = blockIdx.x, h = blockIdx.y, cache = blockIdx.z / a.batch, b = blockIdx.z % a.batch;
    int src = a.src != nullptr ? a.src[b] : (int)((a.src_imm >> (4 * b)) & 15u);
    src = min(max(src, 0), a.batch - 1);
    if (src == b) return;
    int T = a.len != nullptr ? *a.len : a.len_imm;
    T = min(max(T, 0), min(a.t_hi, a.ctx));
    const int p0 = tile * 64;
    if (p0 >= T) return;
    const int n = min(64, T - p0);
    char* const plane = a.base + (size_t)cache * a.cache_stride;
    const size_t so = (((size_t)src * a.heads + h) * a.ctx + p0) * 64, dof = (((size_t)b * a.heads + h) * a.ctx + p0) * 64;  // elements
    const int eb = a.kv_mode == 0 ? 4 : 2;
    const int n16 = n * 4 * eb;  // 16-byte units of n rows of 64 elements: at most 1024
    const u32x4* sp = reinterpret_cast<const u32x4*>(plane + so * eb);
    u32x4* dp = reinterpret_cast<u32x4*>(plane + dof * eb);
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < n16) v[k] = sp[i];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < n16) dp[i] = v[k];
    }
    if (a.kv_mode == 2) {  // the byte plane: n rows of 64 bytes
        const int i = threadIdx.x;
        if (i < n * 4) reinterpret_cast<u32x4*>(plane + a.lo_off + dof)[i] = reinterpret_cast<const u32x4*>(plane + a.lo_off + so)[i];
    }
}

int launch_kv_fork(const KvForkArgs& a, hipStream_t s) {
    ZG_REQUIRE(a.base != nullptr && a.batch >= 1 && a.batch <= 8 && a.heads >= 1 && a.heads < 65536 && a.n_caches >= 1 && a.n_caches * a.batch < 65536 &&
                   a.ctx >= 1 && a.t_hi >= 1 && a.kv_mode >= 0 && a.kv_mode <= 2 && a.cache_stride % 16 == 0 && a.lo_off % 16 == 0,
               ZG_ERR_ARG, "kv fork: bad argument");
    const int tiles = (std::min(a.t_hi, a.ctx) + 63) / 64;
    hipLaunchKernelGGL(kv_fork_kernel, dim3(tiles, a.heads, a.n_caches * a.batch), dim3(256), 0, s, a);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_f32_to_b24(const float* in, size_t rows, int K, void* out, hipStream_t s) {
    if (rows == 0) return ZG_OK;
    ZG_REQUIRE(K % 8 == 0, ZG_ERR_UNSUPPORTED, "f32_to_b24: K=%d must be a multiple of 8", K);
    hipLaunchKernelGGL(f32_to_b24_kernel, dim3(grid_for(rows * (size_t)(K / 8))), dim3(256), 0, s, in, rows, K, reinterpret_cast<char*>(out));
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_b24_split3(const void* in, size_t rows, int K, bf16_t* out, hipStream_t s) {
    if (rows == 0) return ZG_OK;
    ZG_REQUIRE(K % 8 == 0, ZG_ERR_UNSUPPORTED, "b24_split3: K=%d must be a multiple of 8", K);
    hipLaunchKernelGGL(b24_split3_kernel, dim3(grid_for(rows * (size_t)(K / 4))), dim3(256), 0, s, reinterpret_cast<const char*>(in), rows, K, out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_split3(const float* in, size_t rows, int K, bf16_t* out, hipStream_t s) {
    if (rows == 0) return ZG_OK;
    ZG_REQUIRE(K % 4 == 0, ZG_ERR_UNSUPPORTED, "split3: K=%d must be a multiple of 4", K);
    hipLaunchKernelGGL(split3_kernel, dim3(grid_for(rows * (size_t)(K / 4))), dim3(256), 0, s, in, out, rows, K);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

int launch_wte_planes(const void* wte, int weight_type, size_t V, size_t V64, int K, bf16_t* out, hipStream_t s) {
    ZG_REQUIRE(wte && out && V >= 1 && V64 >= V && K % 8 == 0 && (weight_type == WT_F32 || weight_type == WT_B24), ZG_ERR_ARG, "wte planes: bad argument");
    hipLaunchKernelGGL(wte_planes_kernel, dim3(grid_for(V64 * (size_t)(K / 4))), dim3(256), 0, s, wte, weight_type, V, V64, K, out);
    ZG_HIP(hipGetLastError());
    return ZG_OK;
}

}  // namespace zg
