// zg_common.h — shared host/device helpers for libzgpt2_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zgpt2.h"

namespace zg {

// ------------------------------------------------------------------------------ error plumbing
void set_error(const char* fmt, ...);
// Diagnostic: the launchers of the decode kernels note the instantiation they picked (zg_debug_last_kernel; bench.py quotes
// it as the roofline's kernel symbol instead of a hand-kept table).
void note_kernel(const char* fmt, ...);
const char* last_kernel();  // this thread's latest note
int hip_fail(hipError_t e, const char* what, const char* file, int line);
// Test hook ZGPT2_DECODE_PATHS_OFF (bit mask, read per call): the lock-step decode's newer paths switched off so that the paths
// they replaced — still the route of shapes the newer kernels do not take — can be held to the same tokens (tests/test_planes_gpu.py).
// One line per bit: the default path; what the bit restores; when it is read (per plan = every gemv_plan call, at create = zg_gpt_create).
enum DecodePathsOff : int {
    kOffPlanes = 1,            // activation planes between the lock-step kernels; fp32 rows, split by the consumer; at create
    kOffPl4 = 2,               // the four-wave plane-fed Linear; the 16-wave kernel; per plan
    kOffTags = 4,              // tagged hand-overs; tickets; at create
    kOffTileStats = 8,         // LayerNorm statistics by tile from the producer; the consumer's own sums over x; at create
    kOffLineLoads = 16,        // line-shaped weight loads of the 16-wave kernel; fragment-shaped ones; per plan
    kOffLmWpt = 32,            // the wave-per-tile lm_head; the 16-wave kernel in K steps; per plan
    kOffFusedAttn = 64,        // batch 1: ln_1 + c_attn and the attention as one launch (attn_qkv.hip); two launches; at create
    kOffMergeByCount = 128,    // attn c_proj's head merge specialised by split count; the four-slot prologue (gemv_ksplit.hip); per plan
    kOffMergeMlScalar = 256,   // that merge's (m, l) words by wave-uniform loads; by the lanes' own vector loads; per plan
    kAttnTailStoreLast = 512,  // the fused launch's c_attn role stores its tagged word in front of the q / cache store; behind it; at create
    kAttnPollNarrow = 1024,    // its attention role polls the tagged words with 16-byte loads; with 8-byte ones, four per row; at create
};
int decode_paths_off();

#define ZG_HIP(expr)                                                         \
    do {                                                                     \
        hipError_t _e = (expr);                                              \
        if (_e != hipSuccess) return zg::hip_fail(_e, #expr, __FILE__, __LINE__); \
    } while (0)

#define ZG_REQUIRE(cond, code, ...)        \
    do {                                   \
        if (!(cond)) {                     \
            zg::set_error(__VA_ARGS__);    \
            return (code);                 \
        }                                  \
    } while (0)

#define ZG_TRY(expr)             \
    do {                         \
        int _s = (expr);         \
        if (_s != ZG_OK) return _s; \
    } while (0)

// ------------------------------------------------------------------------------ device helpers
typedef uint16_t bf16_t;  // raw bf16 bits
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int kWave = 64;  // CDNA wavefront

__device__ __forceinline__ float bf16_lo(uint32_t packed) { return __uint_as_float(packed << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t packed) {
    return __uint_as_float(packed & 0xFFFF0000u);
}
// fp32 -> bf16, round to nearest even, in integer arithmetic (zg_f32_to_bf16 and the bf16 weight upload: f32_to_bf16_kernel is its one
// caller; the GEMM and decode epilogues convert through cvt_pk_bf16 below, which keeps NaNs by itself).  The rounding increment
// alone would carry a NaN with low payload bits out of its class (0x7FFFFFFF -> -0.0, 0xFFFFFFFF -> +0.0, 0x7F800001 -> +inf): a
// NaN keeps its sign and upper payload and gets the quiet bit, as the hardware conversion leaves it.
__device__ __forceinline__ uint16_t f32_to_bf16_rne(float x) {
    uint32_t b = __float_as_uint(x);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((b >> 16) | 0x0040u);
    b += 0x7FFFu + ((b >> 16) & 1u);
    return (uint16_t)(b >> 16);
}

// B24, the 24-bit KV cache element: the fp32 value rounded (nearest even) to 16 mantissa bits — sign, 8 exponent bits, the 15
// upper mantissa bits — kept as a bf16-shaped upper half in one plane and the next 8 mantissa bits in a byte plane with the
// same element index.  Relative error 2^-17 per element.  b24_round returns the 24 bits right-aligned.
__device__ __forceinline__ uint32_t b24_round(float x) {
    const uint32_t b = __float_as_uint(x);
    uint32_t r = (b + 0x7Fu + ((b >> 8) & 1u)) >> 8;
    // a finite value within 2^-17 of FLT_MAX must not round up to inf (0 x inf would poison masked positions, as the fp16 cache's
    // clamp prevents): one ulp back.  inf / NaN inputs keep their class.
    if ((r & 0x7F8000u) == 0x7F8000u && (b & 0x7F800000u) != 0x7F800000u) r -= 1u;
    return r;
}
__device__ __forceinline__ void b24_store(void* cache, size_t lo_off, size_t elem, float x) {
    const uint32_t r = b24_round(x);
    reinterpret_cast<uint16_t*>(cache)[elem] = (uint16_t)(r >> 8);
    reinterpret_cast<uint8_t*>(cache)[lo_off + elem] = (uint8_t)r;
}

// B24 weights (ZG_GPT_WEIGHTS_B24): every matrix element is b24_round of the fp32 value, stored row-interleaved — row r of an
// [N][K] matrix is [K bf16-shaped upper halves | K low bytes], 3 K r bytes from the matrix base.  A workgroup's rows stay one
// contiguous stretch (the prefetcher's tiles), and K % 64 == 0 keeps every row 16-B aligned.  The type is a tag for the
// templates: its size is what a row costs per element, it is never dereferenced.
struct b24_t {
    uint8_t b[3];
};
// Element (row, k) as the fp32 value it stands for (the decoders of one element: ln_fold, embeddings, plane split)
__device__ __forceinline__ float b24_elem(const void* W, size_t row, int K, size_t k) {
    const uint8_t* r = reinterpret_cast<const uint8_t*>(W) + row * (size_t)(3 * K);
    return __uint_as_float(((uint32_t)reinterpret_cast<const uint16_t*>(r)[k] << 16) | ((uint32_t)r[2 * (size_t)K + k] << 8));
}

// Two fp32 values -> packed bf16 pair (round to nearest even), one gfx950 instruction (v_cvt_pk_bf16_f32); lo half = a.
// Through the compiler's own conversion, NOT an asm statement: the hazard recognizer pads nothing around inline asm, and a
// packed pair that an MFMA reads as an operand right behind the conversion was read half-written — alternating groups of four
// B-operand columns kept the old register contents (the pipelined prompt attention, round 5: tools/dbg_attn_all.py).
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{a, b}, bf16x2_t));
}

// Exact three-term bf16 split of two fp32 values: x = hi + mid + lo (24 = 8 + 8 + 8 mantissa bits; every
// residual is exactly representable).  Outputs are packed pairs {x1 : x0}.  11 VALU instructions per pair —
// the integer-emulated rounding it replaces made the split the longest phase of the batched GEMV prologue.
__device__ __forceinline__ void split3_pk(float x0, float x1, uint32_t& hi, uint32_t& mid, uint32_t& lo) {
    hi = cvt_pk_bf16(x0, x1);
    const float r0 = x0 - bf16_lo(hi), r1 = x1 - bf16_hi(hi);
    mid = cvt_pk_bf16(r0, r1);
    lo = cvt_pk_bf16(r0 - bf16_lo(mid), r1 - bf16_hi(mid));
}

// Four consecutive fp32 values as their three bf16 planes: two split3_pk and three 8-byte stores, plane p at o + p * plane_stride
// elements (the row-wise [hi | mid | lo] layout, the plane-major one and a batch row's 32-k step of plane_elem alike)
__device__ __forceinline__ void store_split3x4(bf16_t* o, size_t plane_stride, f32x4 v) {
    uint32_t h0, m0, l0, h1, m1, l1;
    split3_pk(v.x, v.y, h0, m0, l0);
    split3_pk(v.z, v.w, h1, m1, l1);
    *reinterpret_cast<u32x2*>(o) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(o + plane_stride) = u32x2{m0, m1};
    *reinterpret_cast<u32x2*>(o + 2 * plane_stride) = u32x2{l0, l1};
}

// elements [k, k + 4) of row `row` of a B24 matrix [.][K] (k % 4 == 0): one 8-B load of upper halves, one 4-B load of low bytes
__device__ __forceinline__ f32x4 load_b24x4(const void* w, size_t row, int K, int k) {
    const char* r = reinterpret_cast<const char*>(w) + row * (size_t)(3 * K);
    const u32x2 h = *reinterpret_cast<const u32x2*>(r + 2 * (size_t)k);
    const uint32_t l = *reinterpret_cast<const uint32_t*>(r + 2 * (size_t)K + k);
    return f32x4{__uint_as_float((h.x << 16) | ((l & 0xffu) << 8)), __uint_as_float((h.x & 0xffff0000u) | (l & 0xff00u)),
                 __uint_as_float((h.y << 16) | ((l >> 8) & 0xff00u)), __uint_as_float((h.y & 0xffff0000u) | ((l >> 16) & 0xff00u))};
}

// THE order of (value, index) pairs that decides which token a greedy step emits: greater value first, lower index on ties.  A NaN
// never comes before anything.  lm_head's argmax epilogues produce a row's partials under it (gemv_internal.h better), the step head, the
// log-probability stage and the stop stage pick from them under it (sample_common.h wave_first / partials_*), the top-N lists are
// in it (tests/pick_ref.py states it for the tests).
__device__ __forceinline__ bool pick_before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }
// A picked index as a token: anything outside the vocabulary (the start index of a row that held nothing comparable, a corrupted
// record) is token 0 — never an address past a table
__device__ __forceinline__ int clamp_token(int t, int vocab) { return (unsigned)t < (unsigned)vocab ? t : 0; }

// The counter PRNG of (seed, sequence length, row): a splitmix64 finaliser, its upper 24 bits as a uniform in [0, 1).  Integer
// operations and one exact conversion: the host (zg_gpt_sample) and the device (sample_pick_kernel) agree to the bit.
__host__ __device__ inline float counter_uniform(unsigned long long seed, unsigned long long seq_len, unsigned long long b) {
    unsigned long long z = seed * 0x9E3779B97F4A7C15ULL + seq_len * 0xD1B54A32D192ED03ULL + b + 1ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (float)(unsigned)(z >> 40) * 5.9604644775390625e-08f;
}

// Activation planes of the lock-step batch in global memory: the epilogue of the producing kernel writes the exact
// three-term bf16 split of its output row, the consuming Linear loads them as MFMA A fragments — no LDS staging and no
// split in front of its MFMAs.  Element (plane p, batch row m < 8, column k) of a [3][8][K] triple sits at
//   (((k >> 5) * 3 + p) * 8 + m) * 32 + (k & 31)    bf16 elements,
// i.e. the three planes of the 8 rows of one 32-k MFMA step are 1536 contiguous bytes; a triple takes 48 K bytes.
constexpr int kPlaneStep = 3 * 8 * 32;  // elements per 32-k step
__host__ __device__ inline size_t plane_elem(int p, int m, int k) { return ((size_t)((k >> 5) * 3 + p) * 8 + m) * 32 + (k & 31); }
__device__ __forceinline__ void store_planes(bf16_t* pl_out, int m, int k, float v) {  // element (m, k) of an output row as its planes
    uint32_t hi, mid, lo;
    split3_pk(v, 0.0f, hi, mid, lo);
    pl_out[plane_elem(0, m, k)] = (bf16_t)hi;
    pl_out[plane_elem(1, m, k)] = (bf16_t)mid;
    pl_out[plane_elem(2, m, k)] = (bf16_t)lo;
}

// Kernel-argument hygiene of the decode kernels.  Only the first 14 dwords of the arguments are preloaded into SGPRs at
// wave launch (-amdgpu-kernarg-preload-count=16, two of them hold the kernarg pointer); any other field costs a scalar
// load from the kernarg segment, which the compiler issues where the field is first used and waits for on the spot — a
// cold round trip to memory in a real decode step (every launch has its own argument block).  So (1) whatever an
// address of the up-front vector loads depends on travels in the leading arguments, and (2) fields that the tail of a
// kernel needs are touched with ZG_PIN right behind the vector loads: their scalar loads then complete under the vector
// memory latency instead of in the epilogue.
#define ZG_PIN(v) asm volatile("" ::"s"(v))

// DPP row rotate inside each 16-lane row: every lane reads the lane `n` to its right (cyclic).
template <int N>
__device__ __forceinline__ float dpp_row_ror(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), 0x120 | N, 0xF, 0xF, true));
}

// Sum over each 16-lane row; every lane of the row receives the total.
__device__ __forceinline__ float row16_allsum(float v) {
    v += dpp_row_ror<8>(v);
    v += dpp_row_ror<4>(v);
    v += dpp_row_ror<2>(v);
    v += dpp_row_ror<1>(v);
    return v;
}

// Read one lane's value into a scalar register (v_readlane_b32): a few cycles, no LDS crossbar.
__device__ __forceinline__ float lane_value(float v, int lane) {
    return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane));
}

// Sum over groups of LPR consecutive lanes (LPR in {16, 32, 64}); all lanes get the total.
// Rows are combined through v_readlane (scalar broadcast) rather than ds_bpermute: the LDS crossbar
// costs ~100+ cycles of dependent latency per hop, which dominated the small latency-bound kernels.
template <int LPR>
__device__ __forceinline__ float group_allsum(float v) {
    v = row16_allsum(v);
    if (LPR == 32) {
        const float lo = lane_value(v, 0) + lane_value(v, 16), hi = lane_value(v, 32) + lane_value(v, 48);
        v = (threadIdx.x & 32) ? hi : lo;
    }
    if (LPR == 64) v = (lane_value(v, 0) + lane_value(v, 16)) + (lane_value(v, 32) + lane_value(v, 48));
    return v;
}

__device__ __forceinline__ float wave_allsum(float v) { return group_allsum<64>(v); }

__device__ __forceinline__ float wave_allmax(float v) {
    v = fmaxf(v, dpp_row_ror<8>(v));
    v = fmaxf(v, dpp_row_ror<4>(v));
    v = fmaxf(v, dpp_row_ror<2>(v));
    v = fmaxf(v, dpp_row_ror<1>(v));
    return fmaxf(fmaxf(lane_value(v, 0), lane_value(v, 16)), fmaxf(lane_value(v, 32), lane_value(v, 48)));
}

// gelu of src/ops.zig:221-228: 0.5 x (1 + tanh(u)), u = x * 0.7978845608 * (1 + 0.044715 x^2).
// 0.5 (1 + tanh u) == 1 / (1 + exp(-2u)) exactly; this form keeps relative accuracy in both tails.
__device__ __forceinline__ float gelu_ref(float x) {
    const float u = x * 0.7978845608f * (1.0f + 0.044715f * x * x);
    return x / (1.0f + __expf(-2.0f * u));
}

}  // namespace zg
