// zg_kernels.h — host-callable launchers of the HIP kernels (internal to libzgpt2_hip).
#pragma once
#include "zg_common.h"

namespace zg {

// Device-side decode control block (lives in the model arena; read by kernels so that one
// captured hipGraph replays for every position).
struct StepCtrl {
    int step;      // 0-based decode step s; sequence length T = s + 1 while a step runs
    int seq_len;   // T of the step in flight (written by the embed kernel)
    int mode;      // 0: generate loop (tokens from prompts / previous argmax), 1: forced tokens
    int n_partials;  // number of lm_head argmax partials per sequence (grid of the lm_head GEMV)
};

// ------------------------------------------------------------------------------------ GEMV
enum GemvPrologue { PRO_NONE = 0, PRO_LAYERNORM = 1, PRO_ATTN_MERGE = 2 };
enum GemvEpilogue { EPI_STORE = 0, EPI_RESIDUAL = 1, EPI_GELU = 2, EPI_QKV = 3, EPI_ARGMAX = 4 };
enum WeightType { WT_BF16 = 0, WT_F32 = 1, WT_B24 = 2 /* zg_common.h b24_t: rows of [K upper halves | K low bytes] */ };

constexpr int kAttnChunk = 256;       // KV positions per attention workgroup (4 waves x 64)
constexpr int kPartStride = 64 + 2;   // floats per attention partial: o[hd<=64], m, l

struct GemvArgs {
    // y[m][n] = epilogue( sum_k prologue(x)[m][k] * W[n][k] + bias[n] ),  m < M, n < N
    const void* W;  // [N][K], bf16 bits, fp32 or B24 rows, K contiguous (ops.Linear.weight layout)
    const float* bias;  // [N] or nullptr
    int N, K, M;
    // The layout: written by launch_gemv from the GemvPlan just before the launch (kslices below too); no caller reads or writes
    // them.  waves_per_wg < 0: the 16-wave kernel's partial tiles alias its planes (GemvPlan.alias).
    int rows_per_wave;
    int waves_per_wg;
    int prologue, epilogue;
    // PRO_NONE / PRO_LAYERNORM input
    const float* x;  // [M][x_stride]
    int x_stride;
    const float* ln_g;
    const float* ln_b;
    float eps;
    // PRO_LAYERNORM, M == 1: the LayerNorm folded out of the dot product (launch_ln_fold): c2[n] = sum_k W g,
    // c3[n] = sum_k W b + bias[n]; null = use the kernel that normalises the input first
    const float* ln_c2;
    const float* ln_c3;
    // PRO_ATTN_MERGE input: partials [M][H][max_splits][kPartStride]
    const float* part;
    int n_heads, head_dim, max_splits;
    const StepCtrl* ctrl;  // seq_len for the merge / KV scatter position
    int t_hi;  // launch-time upper bound of seq_len (same 256-position chunk as seq_len); 0 = read ctrl
    // EPI_STORE / EPI_RESIDUAL / EPI_GELU
    float* y;
    int y_stride;
    const float* resid;  // may alias y
    int resid_stride;
    // EPI_QKV: q [M][E]; caches [M][H][ctx][hd]
    float* q;
    void* k_cache;
    void* v_cache;
    int ctx;
    int kv_mode;   // 0 fp32, 1 fp16, 2 B24 (bf16 plane + byte plane `kv_lo` bytes further on)
    size_t kv_lo;
    // EPI_ARGMAX: optional logits [M][logits_stride]; partials [M][gridDim.x]
    float* logits;
    int logits_stride;
    float* part_val;
    int* part_idx;
    // split-K over workgroups (batched wide Linears): combine workspace [sk_tiles][4][128] floats and FOUR counters per
    // tile (zero between launches: the last arriver resets its counter; the 16-wave kernel uses counter [tile], the
    // four-wave plane-fed kernel one per wave, [4 tile + wave]); kslices is written by launch_gemv (see rows_per_wave)
    float* sk_ws;
    int* sk_cnt;
    int sk_tiles;
    int kslices;
    // lock-step batch on the matrix cores: activation planes in global memory (zg_common.h plane_elem).  pl_in: the
    // input rows arrive as planes written by the previous kernel (PRO_LAYERNORM: planes of g * x, x itself is read for
    // the row statistics only; PRO_NONE: planes of x).  pl_out: this kernel's output rows (after residual / GELU) are
    // also written as planes, scaled by pl_g[n] when given (the next LayerNorm's gain); EPI_GELU with y == nullptr
    // writes only the planes.
    const bf16_t* pl_in;
    bf16_t* pl_out;
    const float* pl_g;
    // K slices of the four-wave plane-fed kernel meet by TAGGED DATA instead of tickets: slices 1.. store (value, tag) as one
    // 8-byte word, slice 0 polls until the tags are this launch's — one memory-side round trip instead of three.
    // tag = *epoch << 8 | launch_id: epoch is advanced by the embed kernel at every step, launch_id (1..255) is unique
    // among the launches of a step that share sk_tag [sk_tiles][4][128].
    const unsigned* epoch;
    unsigned launch_id;
    unsigned long long* sk_tag;
    unsigned* fault;  // set to 1 by a poller whose bounded wait ran out (the host fails the call loudly: api_gpt.hip check_fault)
    unsigned spin_limit;  // polls before a poller gives up (2^20; ZGPT2_TAG_SPIN_LIMIT for the test of the failure path)
    // LayerNorm statistics by tile: a producer of x (four-wave plane-fed kernel, embed kernel) also writes, per 16-column tile
    // and batch row, the sum and the sum of squares of its 16 outputs, st_out [8][N / 16][2]; the LayerNorm-fed consumer
    // adds the tiles (st_in) instead of reading x again — a third of its vector-memory traffic
    float* st_out;
    const float* st_in;
    const float* zero;        // device pointer to a few zero floats (stand-in for absent bias / residual)
    unsigned long long* dbg;  // diagnostic timestamps (only read by -DZG_STAMPS builds)
    unsigned* progress;       // launch counter followed by the side-stream prefetcher (prefetch.hip); null = not counted
};

// Which kernel a decode-regime Linear takes and how it is laid out: decided once per launch by gemv_plan (gemv.hip holds every
// shape threshold), carried out by launch_gemv.  Callers read the outcome here instead of asking shape questions of their own.
enum GemvRoute {
    GR_VALU = 0,         // gemv_kernel: any prologue / epilogue, M <= 8 rows in LDS
    GR_VALU_GROUPS = 1,  // the same in row groups of row_group rows that fit the LDS (plain Linears: the rows are independent)
    GR_GENERIC = 2,      // K % 8 != 0: one wave per row, plain Linear only
    GR_KSPLIT = 3,       // M == 1, wide plain input or the head merge: the four waves split K
    GR_LNK = 4,          // M == 1, LayerNorm folded out of the dot product
    GR_MFMA16 = 5,       // 2..8 rows on the matrix cores: 16 waves (4 for lm_head)
    GR_MFMA16_KS = 6,    // ... in four K slices over as many workgroups
    GR_PL4 = 7,          // plane-fed four-wave kernel
    GR_PL4_KS = 8,       // ... in four K slices
    GR_LM_WPT = 9,       // lm_head, one wave per tile
};
struct GemvPlan {
    int route;
    int grid, kslices;  // dim3(grid, kslices)
    int block;          // threads per workgroup
    int lds;            // dynamic LDS bytes
    // the instantiation of the route's kernel
    int mt, lpr, cpl;   // VALU / K split / lnk: batch rows held (1, 2, 4, 8), lanes per row, 16-byte chunks per lane
    int ks, nw;         // 16-wave kernel: 32-k steps per wave (its template bound) and waves
    bool line, gpl, alias;  // ... line-shaped weight loads, input planes from global memory, partial tiles alias the planes
    int pairs;          // plane-fed kernel: 64-k pairs per wave and slice
    int steps;          // wave-per-tile lm_head: 32-k steps per tile
    // what launch_gemv writes into GemvArgs
    int rows_per_wave;  // rows per wave, or 16-row tiles per workgroup on the matrix cores
    int waves_per_wg;
    int row_group;      // GR_VALU_GROUPS: rows per group (each group is laid out on its own; the other fields describe the first)
    // the prefetcher's view (api_gpt_step.hip emit_gemv): workgroup b reads rows b * rows_per_wg .. of W (0 = another mapping), in
    // pf_tiles tiles — on GR_KSPLIT / GR_LNK still the VALU layout's workgroup count, as its job table has always had it, not `grid`
    int rows_per_wg, pf_tiles;
    bool supported;         // launch_gemv runs it
    bool can_take_planes;   // may take its input rows as planes (GemvArgs.pl_in)
    bool can_write_planes;  // may write its output rows as planes (GemvArgs.pl_out)
    bool pl4_with_planes;   // given input planes it runs as the four-wave kernel (the one that reads / writes the tile statistics)
    // launcher matters of GR_KSPLIT's head merge (not among the fields zg_debug_gemv_plan reports): the four-slot prologue that
    // serves any split count instead of the one specialised by it (ZGPT2_DECODE_PATHS_OFF kOffMergeByCount), and the specialised one's
    // (m, l) words through the lanes' vector loads instead of wave-uniform ones (kOffMergeMlScalar)
    bool merge_generic, merge_ml_vector;
};
// Pure host code: no HIP call, no allocation.  Reads ZGPT2_DECODE_PATHS_OFF once (per call: tests flip it between handles).
GemvPlan gemv_plan(const GemvArgs& a, int weight_type);
int launch_gemv(const GemvArgs& a, const GemvPlan& p, int weight_type, hipStream_t s);
int launch_ln_fold(const void* W, int weight_type, const float* g, const float* b, const float* bias, int N, int K, float* c2,
                   float* c3, hipStream_t s);

// ------------------------------------------------------------------------------------ attention
struct AttnArgs {
    const float* q;  // [B][H*hd]
    const void* k;   // element (b,h,t,d) at b*stride_b + h*stride_h + t*stride_t + d
    const void* v;
    long stride_b, stride_h, stride_t;
    int kv_mode;   // 0 fp32, 1 fp16, 2 B24: bf16 plane at k / v, byte plane (same element strides) kv_lo bytes further on
    size_t kv_lo;
    int n_heads, head_dim, batch;
    const StepCtrl* ctrl;  // seq_len read from ctrl->seq_len when non-null
    int seq_len;           // used when ctrl == nullptr
    int t_hi;              // launch-time upper bound of seq_len in the same 64-position bucket (>= seq_len)
    int max_splits;
    float* part;  // [B][H][max_splits][kPartStride]
    unsigned* progress;  // see GemvArgs
    // lock-step batch with activation planes: the last split of (b, h) to arrive merges them and writes the head's output as
    // planes [3][8][H * 64] (plane_elem) for the c_proj Linear; merge_cnt = one zeroed counter per (b, h)
    bf16_t* pl_out;
    int* merge_cnt;
    // ... or, with part_tag [B][H][max_splits][66] given, split 0 merges: the other splits store (value, tag) words and
    // split 0 polls them (see GemvArgs.sk_tag for the tag)
    const unsigned* epoch;
    unsigned launch_id;
    unsigned long long* part_tag;
    unsigned* fault;  // see GemvArgs.fault
    unsigned spin_limit;
    // ZGPT2_DECODE_PATHS_OFF kAttnTailStoreLast as the handle read it at create: the A/B switch of the producer side of
    // the fused launch's hand-over (gemv_lnk_body TAGGED); likewise kAttnPollNarrow, the consumer side
    unsigned tail_off;
    unsigned long long* dbg;  // diagnostic timestamps of the fused launch's attention role (only read by -DZG_STAMPS builds)
};
constexpr unsigned kStepPathsAtCreate = kAttnTailStoreLast | kAttnPollNarrow;  // (zg_common.h DecodePathsOff)
int launch_attn_decode(const AttnArgs& a, hipStream_t s);
// One sequence, fp32 cache, head_dim 64, c_attn on the LayerNorm-folding kernel: ln_1 + c_attn + KV append (g, EPI_QKV) and the
// attention (at) of the same layer in one launch (attn_qkv.hip).  q and the new k / v row reach the attention workgroups as
// (value, tag) words in qkv_tag [3 E], tag = *epoch << 8 | at.launch_id; a timed-out wait raises at.fault.  Same results,
// bit for bit, as launch_gemv + launch_attn_decode.
bool attn_qkv_ok(const GemvArgs& g, const GemvPlan& p, const AttnArgs& at);  // p = gemv_plan(g, ...)
int launch_attn_qkv(const GemvArgs& g, const GemvPlan& p, int weight_type, const AttnArgs& at, const unsigned* epoch, unsigned long long* qkv_tag, hipStream_t s);
// the op tier's general path for head_dim != 64 (fp32, one workgroup per (sequence, head))
int launch_attn_any_dim(const float* q, const float* k, const float* v, long stride_b, long stride_h, long stride_t, int batch, int n_heads,
                        int head_dim, int seq_len, float* out, hipStream_t s);
// Standalone merge (op tier): out[b][h*hd+d] = sum_s w_s o_s / sum_s w_s l_s
int launch_attn_merge(const float* part, int batch, int n_heads, int head_dim, int max_splits,
                      int seq_len, float* out, hipStream_t s);

// ------------------------------------------------------------------------------------ elementwise
int launch_epoch_bump(unsigned* epoch, hipStream_t s);  // measurement chains: advance the tag epoch (api_gpt_debug.hip zg_gpt_time_kernel)
int launch_epoch_add(unsigned* epoch, unsigned n, hipStream_t s);  // tests: n steps at once (api_gpt_debug.hip zg_debug_gpt_age)
// The completion word of an op-tier call, offered to the call's last launch (zg_runtime.h Call::reserve): flag == nullptr offers
// nothing; a launch that stores the word itself (a one-workgroup grid) sets taken, otherwise the caller's one-thread launch follows.
struct DoneSlot {
    unsigned* flag;
    unsigned seq;
    bool taken;
};
int launch_layernorm(float* x, int rows, int n, const float* g, const float* b, float eps, hipStream_t s, DoneSlot* done = nullptr, float* shadow = nullptr);
int launch_gelu(float* x, size_t n, hipStream_t s, DoneSlot* done = nullptr, float* shadow = nullptr);
int launch_softmax(float* x, size_t n, hipStream_t s, DoneSlot* done = nullptr);
int launch_done_flag(unsigned* flag, unsigned seq, hipStream_t s);
struct CopySegs {  // up to four device -> pinned-host segments (16-byte aligned, multiples of 4 bytes)
    const void* src[4];
    void* dst[4];
    unsigned bytes[4];
    int n;
};
int launch_copy_out_done(const CopySegs& segs, unsigned* flag, unsigned seq, hipStream_t s);
int launch_copy2_f32(const float* a, float* da, const float* b, float* db, size_t n, hipStream_t s);
int launch_embedding(const float* w, size_t emb_dim, const size_t* idx, size_t n_idx, size_t n_rows,
                     float* out, int* d_oob_flag, hipStream_t s, DoneSlot* done = nullptr);
int launch_split_qkv(const float* in, size_t rows, size_t n_embed, size_t split_idx, float* out, hipStream_t s);
int launch_transpose(const float* in, size_t batch, size_t t, size_t n, size_t h, float* out, hipStream_t s);
int launch_copy_f32(const float* in, float* out, size_t n, hipStream_t s);
int launch_f32_to_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s);
// fp32 [rows][K] -> bf16 [rows][3K] = [hi | mid | lo], hi + mid + lo == x exactly
int launch_split3(const float* in, size_t rows, int K, bf16_t* out, hipStream_t s);
// fp32 [rows][K] -> B24 rows (b24_round; zg_common.h b24_t), K a multiple of 8
int launch_f32_to_b24(const float* in, size_t rows, int K, void* out, hipStream_t s);
// B24 matrix [rows][K] -> plane-major bf16 [3][rows K], the split launch_split3(values, 1, rows K) makes of the values it holds
int launch_b24_split3(const void* in, size_t rows, int K, bf16_t* out, hipStream_t s);
// wte [V][K] (fp32 or B24) -> its exact bf16 planes, plane-major [3][V64][K] with zero rows behind row V - 1: the weight operand of
// the scoring lm_head on handles whose whole-prompt GEMMs read weight planes
int launch_wte_planes(const void* wte, int weight_type, size_t V, size_t V64, int K, bf16_t* out, hipStream_t s);
// rows [from_row, ctx) of every (cache, sequence x head) strip set to zero: n_caches caches cache_stride bytes apart, each holding a
// plane of [strips][ctx] rows of row_bytes at plane_off (api_gpt.hip clear_kv: what a new sequence must not inherit)
int launch_kv_clear_tail(void* base, int n_caches, size_t cache_stride, size_t plane_off, int row_bytes, int strips, int ctx, int from_row,
                         hipStream_t s);
// Row b of every cache becomes a copy of row src[b] over positions [0, len) (zg_gpt_kv_fork).  The caches are n_caches blocks
// cache_stride bytes apart from base, each [batch][heads][ctx][64] elements of 4 (kv_mode 0) or 2 bytes, with kv_mode 2's byte plane
// of the same element strides lo_off bytes further on.  The grid is fixed by the bucket bound t_hi (a multiple of 64 at or above
// len); the table and the length come from device memory (src, len), or, where those are null, by value: src_imm holds four bits per
// row, len_imm the length.  PRECONDITION: every source is its own source (src[src[b]] == src[b]): then no workgroup reads what
// another writes.
struct KvForkArgs {
    char* base;
    size_t cache_stride, lo_off;
    int n_caches, batch, heads, ctx, kv_mode, t_hi;
    const int* src;
    const int* len;
    unsigned src_imm;
    int len_imm;
};
int launch_kv_fork(const KvForkArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------ MFMA GEMM
// C[M,N] = A[M,K] * B[N,K]^T (+ bias) (optional GELU); bf16 operands, fp32 accumulate; C bf16 or fp32.
int launch_gemm_bf16_nt(const bf16_t* A, const bf16_t* B, const float* bias, void* C, int M, int N, int K, int ldc,
                        bool gelu, bool out_bf16, hipStream_t s);
// The same kernel over a list of (A plane, B plane) pairs: A is [M][lda] holding planes of K = 64 kpp columns each
// (plane p at column p K), B is [N][ldb] likewise; C = sum over pairs of A_plane[pa] * B_plane[pb]^T (+ bias).
// fp32 operands split exactly into bf16 hi + mid + lo planes make the bf16 matrix cores deliver fp32-grade
// products (every bf16 x bf16 product is exact in fp32): planes {(2,0),(1,0),(0,0)} for exact-bf16 weights,
// six pairs for arbitrary fp32 weights.  Pair i's planes sit in bits [4i, 4i + 4) of pa_bits / pb_bits.
struct GemmPlanes {
    int lda, ldb;  // row lengths in elements
    int kpp;       // K-steps (of 64) per plane
    int npairs;
    unsigned pa_bits, pb_bits;
    bool b_plane_major;  // B's planes are whole [N][ldb] matrices one behind the other (the model's fp32-weight planes), not column blocks of a row
};
int launch_gemm_planes(const bf16_t* A, const bf16_t* B, const float* bias, void* C, int M, int N, const GemmPlanes& pl,
                       int ldc, bool gelu, bool out_bf16, hipStream_t s);
int launch_gemm_s4(const bf16_t* A, const bf16_t* B, const float* bias, void* C, int M, int N, const GemmPlanes& pl, int ldc,
                   bool gelu, bool out_bf16, int bn, hipStream_t s);  // gemm_s4.hip
bool gemm_s4_args_ok(const GemmPlanes& pl, int ldc);            // the bounds of gemm_s4_kernel's packed arguments
// The launch of the persistent kernel's 192-wide instantiation (NT = 3: the only one launched) over `items` 256 x 192 tiles (x K
// slices) in tiles_n tile columns: at most wg_cap workgroups, each walking a range of the tile order in column bands `band` tiles
// wide; lds = that instantiation's dynamic LDS bytes (what a plan reports; the launch takes them from the kernel's own traits)
struct S4Grid {
    int grid, band, lds;
};
int gemm_s4_wg_cap();  // 256, or ZGPT2_GEMM_WGS (tests: few workgroups, many tiles each)
S4Grid gemm_s4_grid(int items, int tiles_n, int wg_cap);
// ... and its epilogue kinds for the whole-prompt Linears (gemm_s4.hip; PrefillQkv, PrefillGemmPlan below)
enum { S4_PLAIN = 0, S4_PARTIAL = 1, S4_QKV = 2, S4_SPLIT3 = 3 };
struct PrefillQkv;
struct PrefillGemmPlan;
int launch_gemm_s4_prefill(const bf16_t* A, const bf16_t* W, const float* bias, void* C, int M, int N, const PrefillGemmPlan& p, const PrefillQkv* qkv,
                           hipStream_t s);
int gemm_s4_stamps(unsigned long long* out, size_t n_words);  // diagnostic (ZGPT2_GEMM_DBG bit 256)
int gemm_s4_fault(unsigned* out);  // 1: a stream-K consumer of gemm_s4 gave up waiting for its producer since the last call (results wrong)
int gemm_debug_stamps(unsigned long long* out, size_t n_words);  // of the kernel generation launched last
unsigned long long gemm_mfma_launch_count();  // launches of the persistent MFMA GEMMs so far (tests assert the path taken)
void gemm_note_launch();

// ------------------------------------------------------------------------------------ prefill (prefill.hip)
// Whole-prompt forward.  Activations feeding a GEMM are fp32 split exactly into kSplit bf16 terms,
// stored as planes [M][kSplit * K] = [hi | mid | lo].
constexpr int kSplit = 3;
enum PrefillEpilogue { PF_F32 = 0, PF_RESID = 1, PF_GELU_SPLIT = 2, PF_PARTIAL = 3 /* internal: split-K slice */, PF_QKV = 4 };
// x[b P + t] = wte[tokens[b][pos0 + t]] + wpe[pos0 + t]
int launch_embed_prefill(const int* tokens, int token_stride, int B, int P, const void* wte, const void* wpe,
                         int weight_type, int E, float* x, hipStream_t s, int pos0 = 0);
int launch_ln_split(const float* x, int M, int E, const float* g, const float* b, float eps, bf16_t* out, hipStream_t s);
// C = A[M][kSplit K] * W[N][K]^T + bias; PF_F32: fp32 C[M][ldc]; PF_RESID: C += ...; PF_GELU_SPLIT: bf16 C[M][kSplit N] = split(gelu(...))
// ws: fp32 workspace for split-K partial sums (used when the output has too few tiles to fill the chip).
// ln (PF_RESID only, may be null): LayerNorm of the updated rows, written as split planes to ln->out — fused
// into the split-K tail when there is one, a separate launch_ln_split otherwise.
// PF_QKV: fp32 store of the qkv rows (row m = b P + t) AND the cache append of ops.zig:152-157 for the K / V
// columns, into the head-major caches [b][h][ctx][64] (fp32 or fp16).
struct PrefillQkv {
    int P, E, H, ctx, kv_mode;
    void* k_cache;
    void* v_cache;
    size_t kv_lo;  // kv_mode 2: byte offset of the low-mantissa plane
    // stream-K hand-over of the persistent GEMM (gemm_s4.hip, S4_QKV with 1.5 rounds of tiles): workspace for the producers'
    // accumulators (196608 B per shared tile), one flag word per (shared tile, wave), the launch's epoch (flags of earlier
    // launches are smaller); null = whole tiles only
    void* sk_ws = nullptr;
    size_t sk_ws_bytes = 0;
    unsigned* sk_flags = nullptr;
    unsigned sk_flags_words = 0;  // words behind sk_flags (4 per shared tile: G / 2 tiles for G workgroups)
    unsigned sk_epoch = 0;
    int pos0 = 0;  // a continuation (zg_gpt_extend): row t of a sequence is position pos0 + t, and that is its cache row
};
struct PrefillLn {
    const float* g;
    const float* b;
    float eps;
    bf16_t* out;
};
constexpr int kWeightPlanes = 33;
// A forced route (tests, measurements; zg_debug_prefill_route in include/zgpt2.h): kernel 0 = the library's rule; slices > 0 = the K slices of a residual Linear
struct PrefillForce {
    int kernel, slices;
};
// How one whole-prompt Linear runs: decided once per launch by prefill_gemm_plan (prefill.hip holds every threshold and all of the
// slice, tile and stream-K arithmetic), carried out by launch_prefill_gemm, which derives nothing again.
struct PrefillGemmShape {
    int M, N, K, ldc, epi, nsplit;  // nsplit: 2, kSplit or kWeightPlanes
    size_t ws_floats;
    bool have_ws, have_ln;
    int qkv_e;                       // PrefillQkv.E (0 = none given) and its stream-K operands
    bool have_sk_ws, have_sk_flags;
    size_t sk_ws_bytes;
    unsigned sk_flags_words;
    PrefillForce force;
};
enum PrefillFamily { PFF_S4 = 1 /* gemm_s4_kernel */, PFF_T128 = 2 /* prefill_gemm_kernel */, PFF_T128_WP = 3 /* prefill_gemm_wp_kernel: fp32 weights */ };
enum PrefillTail { PFT_NONE = 0, PFT_LN_SPLIT = 1, PFT_REDUCE = 2, PFT_REDUCE_LN_SPLIT = 3, PFT_REDUCE_RESID_LN = 4 };
struct PrefillGemmPlan {
    int status;       // ZG_OK, or the refusal (then `why` says it and nothing else is set)
    const char* why;
    int family;
    int s4_kind;      // PFF_S4: the epilogue kind, and S4_QKV with the half-tile hand-over
    bool stream_k;
    int ns, nspl;     // 128-row kernels: 64-column strips per wave (tile = 128 x 128 ns), activation planes multiplied (0 on PFF_T128_WP)
    bool partial;     // the GEMM writes fp32 slabs to the workspace and the tail finishes (always so on PFF_T128_WP)
    int grid_x, grid_y, block, lds;
    int slices, slabs;      // K slices of the GEMM; slabs the tail sums (PFF_T128_WP: three passes per slice)
    int xcd_rows, tiles_n;  // 128-row kernels: the packed tp word (prefill_gemm_body)
    int band, s4_ldc;       // PFF_S4: tile-order band width, row length of its output, the plane pairs of its K loop
    GemmPlanes planes;
    int tail;
};
// Pure host code: no HIP call, no allocation.  Reads ZGPT2_GEMM_WGS once (per call: tests flip it between launches).
PrefillGemmPlan prefill_gemm_plan(const PrefillGemmShape& sh);
// force: null = the process-wide pin of prefill_force_route (zg_debug_prefill_route)
int launch_prefill_gemm(const bf16_t* A, const bf16_t* W, const float* bias, void* C, int M, int N, int K, int ldc, int epi,
                        float* ws, size_t ws_floats, const PrefillLn* ln, hipStream_t s, const PrefillQkv* qkv = nullptr,
                        int nsplit = kSplit,  // nsplit = 2: multiply the hi + mid planes only (2/3 of the matrix work);
                                              // kWeightPlanes: W is the plane-major three-term split [3][N][K] of an fp32 matrix
                        const PrefillForce* force = nullptr,
                        PrefillGemmPlan* plan_out = nullptr);  // plan_out (zg_debug_gpt_pass_taps): receives the plan the launch used
// The ZG_PREFILL_PLAN_INTS (21) ints zg_debug_prefill_plan and zg_debug_gpt_pass_taps report of a plan (include/zgpt2.h lists them)
inline void prefill_plan_ints(const PrefillGemmPlan& p, int* v) {
    const GemmPlanes& pl = p.planes;
    const int w[21] = {p.status, p.family, p.tail, p.partial, p.grid_x, p.grid_y, p.block, p.lds, p.slices, p.slabs, p.ns, p.nspl, p.xcd_rows,
                       p.tiles_n, p.s4_kind, p.stream_k, p.band, pl.npairs, (int)pl.pa_bits, (int)pl.pb_bits, pl.b_plane_major};
    for (int i = 0; i < 21; ++i) v[i] = w[i];
}
void prefill_force_route(int kernel, int slices);  // zg_debug_prefill_route: pin the route of every whole-prompt Linear of the process
// Where the prompt attention reads K and V: the k / v columns of the qkv rows (k == nullptr; a whole prompt only), or head-major
// caches [b][h][ctx][64] in storage format fmt (0 fp32, 1 fp16, 2 B24 with its byte plane kv_lo bytes behind the bf16 plane)
struct PrefillKv {
    const void* k = nullptr;
    const void* v = nullptr;
    int fmt = 0;
    size_t kv_lo = 0;
    int ctx = 0;
};
// out[M][kSplit E] = split(causal attention of the P rows per sequence of qkv[M][3E]), M = B P rows ordered (b, t), at positions
// pos0 .. pos0 + P - 1 behind pos0 cached ones (attn_prefill.hip: bf16 matrix cores on exact plane splits; ws = fp32 workspace for
// the partials of split key ranges; force_tiles: key tiles per workgroup, tests; ran_out (zg_debug_gpt_pass_taps): receives the
// geometry word (key tiles per range | max splits << 8 | groups << 16), the kernel (0 whole-prompt, 1 + fmt: the continuation
// kernel of that cache format) and whether the merge kernel ran)
int launch_attn_prefill(const float* qkv, bf16_t* out, int B, int pos0, int P, int E, int H, float* ws, size_t ws_floats, const PrefillKv& kv,
                        hipStream_t s, int force_tiles = 0, int* ran_out = nullptr);

// ------------------------------------------------------------------------------------ step head and sampler stages (sample.hip)
// GPT.sample tail: in-place softmax(logits / temp) per sequence + inverse-CDF draw with uniform u[b].
// part_val / n_part / part_stride: the per-workgroup maxima lm_head's argmax epilogue left (the row maximum without a pass over the
// logits); seg_ws: sample_workspace_floats(batch) floats; write_probs: leave softmax(logits / temp) in the logits rows.
// params null: `temp` for every row, by value (nothing is staged for a uniform call); else params[b].inv_temp of device memory
struct SampleParams;
int launch_sample(float* logits, int batch, int vocab, const SampleParams* params, float temp, const float* u, const float* part_val, int n_part,
                  int part_stride, float* seg_ws, int* token_out, bool write_probs, hipStream_t s);
size_t sample_workspace_floats(int batch);

// Decode-step head kernel: token selection (+ argmax finalisation of the previous step) and
// x = wte[token] + wpe[pos].
struct EmbedArgs {
    // these nine (14 dwords) are what the first loads of the kernel depend on: launch_embed_step hands them to the kernel as
    // leading scalar parameters, which are preloaded into SGPRs (zg_common.h ZG_PIN) — a by-value block never is
    StepCtrl* ctrl;
    const float* part_val;   // [B][n_partials]
    const int* part_idx;
    int part_stride;
    int n_partials;          // lm_head grid size
    const int* prompt;       // [B][prompt_stride]
    const int* prompt_len;   // [B]
    int batch;
    int prompt_stride;
    // ... the rest the kernel reads from the block it is passed, fetched from the kernarg segment under those loads
    const int* forced;       // [B] (mode 1)
    const void* wte;  // [V][E] bf16, fp32 or B24
    const void* wpe;  // [ctx][E]
    int weight_type;
    int n_embed, vocab;
    int* cur_token;          // [B]
    int* out_tokens;         // [B][out_stride]
    int out_stride;
    float* x;                // [B][E]
    bf16_t* pl_out;          // optional planes of pl_g * x for the first Linear of the lock-step batch (GemvArgs.pl_in)
    const float* pl_g;
    unsigned* epoch;         // optional step counter behind the tagged hand-overs (GemvArgs.sk_tag): +1 when a step starts
    float* st_out;           // optional LayerNorm statistics by tile of x (GemvArgs.st_in): [8][n_embed / 16][2]
    int finish_only;         // 1: only record the greedy pick of the last step; 2: argmax -> cur_token
    unsigned* progress;      // set to (T << 8) | 1 (and the XCD of this block beside it) when a step starts; the other decode kernels add 1 each
    const int* sampled;      // [B] (mode 2: generate with the sampler) the token sample_step_kernel drew from the previous step's logits
};
int launch_embed_step(const EmbedArgs& a, hipStream_t s);
// GPT.sample's tail (src/main.zig:200-206) inside the generate loop: temperature and seed live in device memory (one captured
// graph serves every call), the uniform of (sequence b, position T) is the library's counter PRNG of (seed, T, b) — what
// zg_gpt_sample uses when it is given no uniforms.  Every launcher below takes an ARRAY of one entry per row, params[b] (DESIGN
// §3.11): a uniform call stages `batch` equal entries; the form of row b — plain, one descent, two, min-p alone — is read off its
// own entry on the device, whatever chain the launch belongs to.
struct SampleParams {
    float inv_temp;
    unsigned top_k;  // 0: off (the truncated sampler only; read on the device, so one captured graph serves every value)
    unsigned long long seed;
    float top_p;     // 1: off
    float min_p_off; // min-p: temp x log(min_p), added to the row maximum for the threshold tau_m (-inf: off; the filtered sampler kernels only)
};
int launch_sample_step(float* logits, int batch, int vocab, const SampleParams* params, const StepCtrl* ctrl, const float* part_val, int n_part,
                       int part_stride, float* seg_ws, int* token_out, hipStream_t s);
// The sampler behind top-k / top-p truncation (sample_filter.h: an exact radix select of the threshold, one launch per 11-bit
// level, then the segment sums / pick / probabilities with weight 0 under the threshold).  n_levels is the CHAIN's, the largest any
// row needs: 3 = ONE filter is on (top-k if params[b].top_k is, else the nucleus), 6 = both (top-k, then the nucleus over what it
// kept); a row that needs fewer passes its state through the launches it has no descent in — the launches are the same for
// every option value, so a captured chain serves them all; 0 = min-p alone: no selection launch, the threshold-aware tail kernels
// with tau = row maximum + params->min_p_off (with 3 or 6 the same threshold is folded into max(tau_k, tau_p)).  params lives in device memory; u (device, [batch]) or, when null, the
// counter PRNG of (params->seed, ctrl->seq_len, b).  fws: filter_workspace_bytes(batch) bytes whose first
// filter_workspace_zeroed_bytes(batch) were zero before the first chain (every chain leaves them so).  write_probs: the
// renormalised probabilities (exact 0 where dropped) are left in the logits rows.
struct FilterWs {
    unsigned long long* mass;  // [batch][3][2048] fixed-point masses by histogram bin
    unsigned* cnt;             // [batch][3][2048] counts
    void* st;                  // [batch][2] descent state
    float* tau;                // [batch] the threshold max(tau_k, tau_p)
};
size_t filter_workspace_bytes(int batch);
FilterWs filter_workspace(void* base, int batch);
int launch_sample_filtered(float* logits, int batch, int vocab, const SampleParams* params, int n_levels, const float* u, const StepCtrl* ctrl,
                           const float* part_val, int n_part, int part_stride, float* seg_ws, const FilterWs& fws, int* token_out, bool write_probs,
                           hipStream_t s);
// part_val[batch][n_part] = maxima of n_part slices of every row (what lm_head's argmax epilogue leaves; zg_debug_sample_rows)
int launch_row_max_partials(const float* logits, int batch, int vocab, float* part_val, int n_part, hipStream_t s);
// Repetition / presence / frequency penalties on the raw logits, in front of either sampler (sample_penalty.h; include/zgpt2.h
// zg_logit_penalties).  Two launches: one workgroup per row counts the row's history in an LDS table and rewrites every logit
// whose index occurs in it, once; then part_val / part_idx [batch][n_part] are rebuilt as the maxima (lowest index on ties) of n_part
// slices of the penalised rows, which is all the samplers and zg_gpt_argmax take from lm_head's argmax epilogue.
// The history of row b: prior[b][0 .. prior_len[b]) followed, when ctrl is given (the generate loop), by
// rec[b][params->past_len .. ctrl->step - 2] — the tokens recorded when the step in flight (ctrl->step - 1) is sampled.  All of it is
// read on the device, so one captured launch serves every position and every value.  max_hist: the longest history a row may have
// (<= kPenMaxHistory: the table of 2 max_hist slots lives in the LDS); anything longer is cut, a token >= vocab is skipped.
// params is an array of one entry per row; a row whose entry is {1, 0, 0} is counted but not rewritten (it keeps its bits).
struct PenParams {
    float repetition, presence, frequency;
    int past_len;  // first recorded position that belongs to the history (generate loop)
};
struct PenHistory {
    const int* prior;      // [batch][prior_stride] or nullptr
    const int* prior_len;  // [batch]
    int prior_stride;
    const int* rec;        // [batch][rec_stride] the loop's token record (with ctrl), or nullptr
    int rec_stride;
    const StepCtrl* ctrl;
    int max_hist;
};
constexpr int kPenMaxHistory = 8192;  // 16384 slots x (key, count) = 128 KB of the 160 KB LDS
// rebuild false: the second launch is left out — for a tail whose edit stage (launch_logit_edit) follows and rebuilds the partials from
// the row it leaves; nothing between the two reads them.
int launch_penalize(float* logits, int batch, int vocab, const PenParams* params, const PenHistory& h, float* part_val, int* part_idx, int n_part,
                    unsigned* counts_out, hipStream_t s, bool rebuild = true);

// Logit bias and token allow / ban lists on the logit row, behind the penalties and in front of either sampler (sample_edit.h;
// include/zgpt2.h zg_logit_edits).  ONE launch, grid (n_part, batch): every workgroup edits one slice of a row — -inf where the keep
// set's bit is clear, x + v where a kept index has a bias — and leaves that slice's maximum (lowest index on ties) in part_val /
// part_idx [batch][n_part], the geometry of launch_penalize's rebuild.  tab (device): the bias pairs, distinct ids; keep (device):
// a bitmap of vocab bits, (vocab + 31) / 32 words.  Count and ids are read on the device and bounds-checked there, so one captured
// launch serves every set.
constexpr int kEditMaxBias = 512;
struct EditTable {
    int n_bias, pad[3];
    int ids[kEditMaxBias];
    float vals[kEditMaxBias];
};
int launch_logit_edit(float* logits, int batch, int vocab, const EditTable* tab, const unsigned* keep, float* part_val, int* part_idx, int n_part,
                      hipStream_t s);

// Guided decoding: a token-level automaton per row (sample_guide.h; include/zgpt2.h zg_guide).  next [n_states][vocab] uint16: the
// state behind picking a token, kGuideDead where the state does not allow it; keep [n_states][(vocab + 31) / 32]: the same as one
// bitmap per state, built by the host; *n_states (device word, <= kGuideMaxStates); state [batch]: where each row stands, negative
// (or >= *n_states) for a row without a guide.  All of it is read on the device and clamped before it becomes an address, so one
// captured launch serves every table.  ctrl / prompt_len: the column in flight is ctrl->seq_len - 1 and row b is guided there only
// when that is a picked column (>= prompt_len[b]); ctrl null: every row stands at a picked column, column 0.
//   launch_guide_mask     the twin of launch_logit_edit (its grid, slices and single-writer rule): -inf where the row's state, ANDed
//                         with the call's keep set when edits are given (tab / keep, both or neither), drops an index; the bias of
//                         a kept index; the slice maxima rebuilt into part_val / part_idx.  A row without a guide and without edits
//                         is only read.
//   launch_guide_advance  one small workgroup behind the sampler: for a guided row at a picked column, rec[b][column] = state[b]
//                         (rec may be null), then state[b] = next[state[b]][picks[b]] unless that is dead or out of range.
constexpr int kGuideMaxStates = 256;       // ZG_GUIDE_MAX_STATES of the header
constexpr unsigned kGuideDead = 0xffffu;   // ZG_GUIDE_DEAD
struct GuideArgs {
    const unsigned short* next;
    const unsigned* keep;
    const int* n_states;
    int* state;
    int* rec;
    int rec_stride;
    const StepCtrl* ctrl;
    const int* prompt_len;
};
int launch_guide_mask(float* logits, int batch, int vocab, const EditTable* tab_or_null, const unsigned* keep_or_null, const GuideArgs& g, float* part_val,
                      int* part_idx, int n_part, hipStream_t s);
int launch_guide_advance(const GuideArgs& g, const int* picks, int batch, int vocab, hipStream_t s);

// History-dependent token bans (sample_ban.h; include/zgpt2.h zg_ban_rules): no-repeat n-grams, multi-token bad words and the
// suppress list of min-tokens, between the penalties and the edits.  BanRules is the device block of a call's rules (one block,
// read on the device and clamped there, so one captured launch serves every rule set): row b's n-gram size and min-tokens, the
// words table, the suppress ids, and past_len — the first recorded position that belongs to the history (generate loop).
// ONE launch, one workgroup of 256 threads per row: the row's history (PenHistory, read IN ORDER: prior, then the loop's record;
// lengths clamped as penalty_apply_kernel clamps them, max_hist <= kPenMaxHistory ints of LDS) goes into the LDS, its suffix is
// compared against every window and every word, and each match stores -inf to its token after a bounds check.  picked of row b:
// ctrl->seq_len - 1 - prompt_len[b] (the loop), or picked[b] (ctrl null: the row harness).  A row whose rules are all off at this
// column returns before it touches anything.  The row-maximum partials are NOT rebuilt here: launch_row_argmax_partials, or the
// edit launch behind it, does that.
constexpr int kBanMaxNgram = 16;     // ZG_BAN_MAX_NGRAM of the header
constexpr int kBanMaxWords = 64;     // ZG_BAN_MAX_WORDS
constexpr int kBanMaxWordLen = 16;   // ZG_BAN_MAX_WORD_LEN
constexpr int kBanMaxSuppress = 16;  // ZG_BAN_MAX_SUPPRESS
constexpr int kBanMaxRows = 64;      // rows of the harness (a handle has at most 8)
struct BanRules {
    int n_words, n_suppress, past_len, pad;
    int ngram[kBanMaxRows];
    int min_tokens[kBanMaxRows];
    int suppress[kBanMaxSuppress];
    int word_len[kBanMaxWords];
    int words[kBanMaxWords][kBanMaxWordLen];
};
struct BanArgs {
    const BanRules* rules;
    const int* prompt_len;  // [batch] (with hist.ctrl), absolute
    const int* picked;      // [batch] (without hist.ctrl)
};
int launch_ban(float* logits, int batch, int vocab, const BanArgs& a, const PenHistory& h, hipStream_t s);
// part_val / part_idx [batch][n_part] rebuilt from the rows as they stand (launch_penalize's second launch, alone)
int launch_row_argmax_partials(const float* logits, int batch, int vocab, float* part_val, int* part_idx, int n_part, hipStream_t s);

// The log-probability stage behind the sampler (sample_logprob.h; include/zgpt2.h zg_gpt_generate_logprobs_enqueue): for every row,
// the log-probability of the token the step records and the *top_n (device memory, 0 .. 20) largest logits with theirs, written
// into column ctrl->seq_len - 1 of the record buffers (ctrl null: column 0) — NaN where that column is below prompt_len[b] (null:
// never).  tokens (device, [batch]): the sampler's draw; null: the lowest-index argmax of part_val / part_idx (greedy).  Two
// launches; part_val as for the samplers.  vocab <= 262144.
struct LogprobWs {
    float* sum;  // [batch][chunks] sum of exp(x - max) by chunk
    float* val;  // [batch][chunks][20] the chunk's largest values, in order
    int* idx;    // ... and their indices
};
struct LogprobRec {
    float* logprob;       // [batch][stride]
    int* top_ids;         // [batch][stride][20]
    float* top_logprobs;  // [batch][stride][20]
    int stride;           // columns of a row (the context)
};
size_t logprob_workspace_bytes(int batch, int vocab);
LogprobWs logprob_workspace(void* base, int batch, int vocab);
int launch_logprob(const float* logits, int batch, int vocab, const float* part_val, const int* part_idx, int n_part, int part_stride, const int* top_n,
                   const LogprobWs& ws, const int* tokens, const StepCtrl* ctrl, const int* prompt_len, const LogprobRec& rec, hipStream_t s);
// The scoring stage behind a whole-prompt pass (sample_score.h; include/zgpt2.h zg_gpt_score): `rows` rows of logits [rows][row_stride]
// (only columns < vocab are read) that are rows tg.row0 .. of a pass of tg.n new positions per sequence behind tg.past cached ones.
// Row t of sequence b predicts position tg.past + t + 1: its target is tg.tokens[b][that position] and column that position of the
// record buffers receives the target's log-probability and the *top_n largest logits with theirs; the last row of a sequence
// writes nothing.  Two launches; the row maximum comes from the chunks.  vocab <= 262144.
struct ScoreWs {
    LogprobWs lp;  // over [rows][chunks]; sum: of exp(x - max[chunk])
    float* max;    // [rows][chunks] the chunk's own maximum, in memory between lp.sum and lp.val
};
struct ScoreTargets {
    const int* tokens;  // [batch][token_stride], indexed by absolute position
    int token_stride;
    int n, past, row0;
};
size_t score_workspace_bytes(int rows, int vocab);
ScoreWs score_workspace(void* base, int rows, int vocab);
int launch_score(const float* logits, int rows, int vocab, int row_stride, const int* top_n, const ScoreWs& ws, const ScoreTargets& tg, const LogprobRec& rec,
                 hipStream_t s);
// The stop stage, last in the tail of a step (sample_stop.h; include/zgpt2.h zg_stop_conditions): one launch, one wave per row
// (batch <= kStopMaxRows).  The conditions live in device memory, so one captured launch serves every set.  finish_col / reason
// [batch]: -1 while a row has none, written once.  host (pinned, optional): progress = column + 1 every launch, done_col = the
// highest finish column + 1 once every row has one — stored by the kernel itself, read by the host without a copy.
constexpr int kStopMaxIds = 16, kStopMaxSeqs = 8, kStopMaxSeqLen = 16, kStopMaxRows = 8;  // ZG_STOP_MAX_* of the header
struct StopConds {
    int n_ids, n_seqs;
    int ids[kStopMaxIds];
    int seq_len[kStopMaxSeqs];
    int seq[kStopMaxSeqs][kStopMaxSeqLen];
};
struct StopHost {
    unsigned progress;  // columns the stage has seen: the last launch's column + 1
    unsigned done_col;  // 0 until every row has finished
};
struct StopArgs {
    const StopConds* conds;
    const int* tokens;       // [batch][stride] the loop's record (columns below the one in flight)
    int stride;
    const int* prompt_len;   // [batch] first picked column of a row
    int batch, vocab;
    const StepCtrl* ctrl;    // the column in flight is ctrl->seq_len - 1 ...
    int col;                 // ... unless this is >= 0 (zg_debug_stop_rows)
    const int* picks;        // [batch] the sampler's draw of this step; null: ...
    int pick_from_record;    // ... tokens[b][column] (zg_debug_stop_rows), or the argmax of the partials (greedy)
    const float* part_val;
    const int* part_idx;
    int n_part, part_stride;
    int* finish_col;
    int* reason;
    StopHost* host;
};
int launch_stop(const StopArgs& a, hipStream_t s);
// The beam stage of a step (sample_beam.h; include/zgpt2.h zg_beam_options): one launch, one workgroup, one wave per group, behind
// the log-probability stage whose top-2W lists of the column in flight it reads.  The options and everything a group carries from
// step to step live in ONE device block, so one captured launch serves every call.  Pool entries and the per-group words are
// indexed by g * W + k: there are never more of them than rows.
constexpr int kBeamMax = 8, kBeamRows = 8;  // ZG_BEAM_MAX; rows of a handle
struct BeamState {
    // the options of the call, staged by the host
    int W;       // beams per group (1 .. kBeamMax)
    int eos;     // the token that ends a hypothesis, -1: none
    int early;   // early_stopping != 0
    int c0;      // the first picked column
    // carried from step to step
    float score[kBeamRows];        // cumulative score of the beam in each slot
    int src[kBeamRows];            // slot each slot's beam came from in the last step: the table of that step's cache fork
    int pool_n[kBeamRows];         // [g]: entries of group g's pool
    int done_col[kBeamRows];       // [g]: the column at which group g was done, -1 while it is not
    float pool_sum[kBeamRows], pool_norm[kBeamRows];  // [g * W + k]
    int pool_parent[kBeamRows], pool_col[kBeamRows];
};
struct BeamArgs {
    BeamState* st;
    const float* lenpow;       // [n_lenpow]: lenpow[L] = (float)pow(L, length_penalty)
    int n_lenpow;
    int batch, vocab;
    const int* top_ids;        // the lists: [batch][stride][20], by the slot as it stood before the step
    const float* top_logprobs;
    int stride;
    const StepCtrl* ctrl;      // the column in flight is ctrl->seq_len - 1 ...
    int col;                   // ... unless this is >= 0 (zg_debug_beam_rows)
    int* sampled;              // [batch] out: the token of the beam now in each slot
    int* parent;               // [batch][stride] out
    float* score;              // [batch][stride] out
    float* logprob;            // [batch][stride] out: the chosen list entry's bits
    StopHost* host;            // pinned, optional: progress / done_col as the stop stage stores them
};
int launch_beam(const BeamArgs& a, hipStream_t s);

// ------------------------------------------------------------------------------------ multi-GPU (dist.hip)
int dist_broadcast(void* buf, size_t bytes, int root, hipStream_t s);  // in place, over the communicator of zg_dist_init

// ------------------------------------------------------------------------------------ decode prefetcher (prefetch.hip)
enum PfKind { PF_NONE = 0, PF_WEIGHTS = 1, PF_KV = 2 };
constexpr unsigned PF_STOP = 0xffffffffu;  // value of the progress word that ends the prefetcher
// What launch `index` of a decode step reads: weights = n_wg contiguous tiles of wg_bytes (block b reads tile b);
// KV = the rows of earlier positions of one layer's caches, laid out for the (heads, splits, batch) attention grid.
struct PfJob {
    const char* base;
    const char* base2;    // PF_KV: the V cache
    size_t total_bytes;   // PF_WEIGHTS: end of the matrix (the last tile may be short)
    unsigned wg_bytes, n_wg;
    unsigned touch_bytes;  // PF_WEIGHTS: leading part of every tile that is fetched (the whole tile unless the matrix is far larger than the L2s)
    unsigned kind;
    unsigned n_heads, ctx, batch, row_bytes;  // PF_KV
    unsigned cls;          // kernel class of the launch (1 c_attn .. 6 lm_head, as in zg_gpt_profile_step)
    unsigned pad;
    // small per-row / per-column vectors every block reads a few lines of (bias, folded-LayerNorm vectors, ln gain):
    // fetched whole into every XCD — once the weights come from the L2 these are what a block would wait for
    const char* aux[3];
    unsigned aux_bytes[3];
    unsigned pad2;
};
struct alignas(8) PfCtl {
    unsigned progress;    // (T << 8) | launches started in the step at sequence length T;  PF_STOP ends the prefetcher
    unsigned base_xcd;    // 0x100 | XCC_ID of block 0 of the step's launches (block b then runs on XCD (base + b) % 8);
                          // written with `progress` as one 64-bit store by the embed kernel
    unsigned sink_guard, sink;
    unsigned ticket[8];       // prefetcher workgroups that found themselves on XCD x
    unsigned exit_reason[8];  // 1 stop, 2 idle limit
    unsigned jobs_done[8];
    unsigned xcd_log[256];    // -DZG_STAMPS builds: 0x100 | XCC_ID of block 0 of launch i of the last step
};
struct PfArgs {
    PfCtl* ctl;
    const PfJob* jobs;  // [njobs]: index 0 = the embed kernel (nothing to fetch), then the step's launches in order
    int njobs;          // launches of a step with lm_head
    int lead;           // launches ahead of the running one
    int nsub;           // prefetcher workgroups per XCD
    int max_T;          // last sequence length of the generation (nothing is fetched for steps beyond it)
    unsigned idle_limit;
    unsigned sleep;     // s_sleep(8) repetitions between polls
    unsigned cls_mask;  // bit c set: launches of class c are fetched for
    unsigned line_shift;  // log2 of the touch stride in bytes (7 = one load per 128-byte line)
    unsigned cap_bytes;   // most bytes fetched for one launch (the head of every tile when the matrix is larger); 0 = no cap
};
int launch_prefetcher(const PfArgs& a, hipStream_t s);

// Every decode kernel counts itself in at entry (one lane of block 0; fire and forget).  A launch that does the work of n
// launches of the job table (the fused ln_1 + c_attn + attention kernel: 2) counts n.
__device__ __forceinline__ void pf_count(unsigned* progress, unsigned n = 1u) {
    if (progress != nullptr && (blockIdx.x | blockIdx.y | blockIdx.z | threadIdx.x) == 0) {
#ifdef ZG_STAMPS
        const unsigned old = __hip_atomic_fetch_add(progress, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        reinterpret_cast<PfCtl*>(progress)->xcd_log[old & 255u] = 0x100u | (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u);
#else
        __hip_atomic_fetch_add(progress, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
}

}  // namespace zg
