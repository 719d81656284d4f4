// attn_qkv.hip — one sequence: ln_1 + c_attn + KV append AND the decode attention of the same layer in one launch.
//
// The step of a decode token is a chain of dependent launches; every layer used to start with two of them: the LayerNorm-fed
// c_attn (gemv_lnk_kernel) and the split-KV attention (attn_decode_kernel<float>).  The attention workgroup of head h needs
// only two things from this step: the 64 q values of head h and, in the split that holds position T - 1, the new k / v row of
// head h.  Its large input — the K / V rows of positions 0 .. T - 2 — was written by earlier steps.  So the two run as one
// launch with a 1-D grid whose role is chosen by block index:
//   blocks [0, G)          the c_attn workgroups, gemv_lnk_body unchanged (LayerNorm fold, q store, KV append), which in
//                          addition store every output as a (value, tag) word into qkv_tag [3 E] (agent-scope relaxed stores);
//   blocks [G, A0)         (padding to a multiple of 8: block b runs on XCD (base + b) % 8, and the prefetcher's KV job places
//                          attention block i as block i of a launch) return at once;
//   blocks [A0, A0 + H S)  the attention workgroups (head h, split s) = A0 + h + H s, attn_decode_body: issue the K / V loads of
//                          the chunk first, then poll the tagged q (and new k / v) words with a bound, then compute exactly as
//                          the standalone kernel and write the partials for the c_proj prologue (PRO_ATTN_MERGE).
// The K / V fetch of the attention workgroups overlaps the c_attn work instead of following it across a launch boundary.
//
// Progress: the attention workgroups wait only for workgroups with LOWER block indices.  Every XCD dispatches its share of the
// grid in block order, so on each XCD all c_attn workgroups of the launch are placed before any of its attention workgroups: a
// waiting workgroup never holds a slot that a producer of its own launch on its own XCD still needs, whether or not the whole grid
// is resident at once (GPT-2 XL: 600 + 100 workgroups of 210 VGPRs against 2 x 256 slots — a second round for c_attn, and still
// 722 against 695 tok/s for two launches; profiles/round7_fused_attn_other_configs.json).  What this argument does not cover are
// OTHER launches: co-running handles on private streams (gpt.GPTGroups) could in principle fill an XCD with their own waiting
// attention workgroups while this launch's producers wait for a slot there.  At 124M a launch has 48 attention workgroups, six
// per XCD, against 64 slots per XCD, and the hardware queues bound how many launches run at once; the argument of
// publish_partial (attn_decode.h) accepts the same residual risk.  The wait is bounded (spin_limit): a poller that runs out
// raises the fault word and the call fails (api_gpt.hip check_fault) — it can never hang the queue or pass silently.
// Tags: tag = *ew << 8 | launch_id — the embed kernel advances the epoch at every step, launch ids are unique per layer.
#include "attn_decode.h"
#include "gemv_internal.h"

namespace zg {

namespace {

struct QkvAttnArgs {
    AttnArgs at;          // the attention role's arguments (q unused; part, fault, spin_limit, launch_id, t_hi ...)
    unsigned sb, sh, st, th;  // packed as for attn_decode_kernel
    const unsigned* ew;   // epoch word
    unsigned long long* qkv_tag;  // [3 E] (value, tag) words
    unsigned a0;          // first attention block
};

// 14 preloaded dwords (zg_common.h ZG_PIN): those of gemv_lnk_kernel, with K in the low and G in the high half of `kg`, so that
// the c_attn role — the one on the critical path — reads its leading arguments as the standalone kernel does.  The attention
// role's arguments come from the kernarg segment; their scalar loads complete well inside the c_attn work it waits for anyway.
template <typename WT, int LPR, int CPL>
__global__ __launch_bounds__(256) void attn_qkv_kernel(const void* __restrict__ Wv, const float* __restrict__ xin, unsigned ne, unsigned kg,
                                                       const float* __restrict__ ln_g, const float* __restrict__ c2,
                                                       const float* __restrict__ c3, const int* __restrict__ cw, const GemvArgs a,
                                                       const QkvAttnArgs f) {
    const unsigned blk = blockIdx.x;
    if (blk < (kg >> 16)) {
        gemv_lnk_body<WT, LPR, CPL, 4, true>((int)blk, Wv, xin, ne, (int)(kg & 0xffffu), ln_g, c2, c3, cw, a, 2u, f.qkv_tag, f.ew,
                                             f.at.launch_id, (f.at.tail_off & kAttnTailStoreLast) == 0);
        return;
    }
    if (blk < f.a0) return;
    const unsigned r = blk - f.a0, H = f.th >> 20;
    attn_decode_body<float, true>((int)(r % H), (int)(r / H), 0, nullptr, f.at.k, f.at.v, f.sb, f.sh, f.st, f.th, cw, f.ew, f.at, f.qkv_tag);
}

}  // namespace

bool attn_qkv_ok(const GemvArgs& g, const GemvPlan& p, const AttnArgs& at) {
    return p.route == GR_LNK && g.epilogue == EPI_QKV && g.M == 1 && g.K <= 0xffff && at.batch == 1 && at.kv_mode == 0 && at.head_dim == 64 &&
           at.stride_t == 64 && at.ctrl != nullptr && at.pl_out == nullptr && at.part_tag == nullptr && g.head_dim == 64 &&
           g.N == 3 * at.n_heads * 64;
}

int launch_attn_qkv(const GemvArgs& g, const GemvPlan& p, int weight_type, const AttnArgs& at, const unsigned* epoch, unsigned long long* qkv_tag,
                    hipStream_t s) {
    ZG_REQUIRE(attn_qkv_ok(g, p, at) && epoch != nullptr && qkv_tag != nullptr && at.launch_id >= 1 && at.launch_id <= 255, ZG_ERR_ARG,
               "fused c_attn + attention: unsupported arguments");
    ZG_REQUIRE(at.t_hi >= 1 && at.t_hi < (1 << 20) && at.n_heads < (1 << 12), ZG_ERR_UNSUPPORTED, "fused attention: t_hi %d / heads %d", at.t_hi,
               at.n_heads);
    const int splits = (at.t_hi + kAttnChunk - 1) / kAttnChunk;
    ZG_REQUIRE(splits <= at.max_splits, ZG_ERR_ARG, "fused attention: t_hi %d needs %d splits > %d", at.t_hi, splits, at.max_splits);
    ZG_REQUIRE(at.stride_b >= 0 && at.stride_h >= 0 && at.stride_h < (1ll << 32), ZG_ERR_UNSUPPORTED, "fused attention: strides beyond 32 bits");
    QkvAttnArgs f{};
    f.at = at;
    f.sb = (unsigned)at.stride_b;
    f.sh = (unsigned)at.stride_h;
    f.st = (unsigned)at.stride_t | 0x80000000u;  // sequence length from the control block
    f.th = (unsigned)at.t_hi | ((unsigned)at.n_heads << 20);
    f.ew = epoch;
    f.qkv_tag = qkv_tag;
    const int* cw = reinterpret_cast<const int*>(g.ctrl);
    // the c_attn role: the row mapping and instantiation of the lnk plan
    const unsigned G = (unsigned)p.grid;
    f.a0 = (G + 7u) & ~7u;
    const unsigned grid = f.a0 + (unsigned)(at.n_heads * splits);
#define ZG_QA(LPR_, CPL_)                                                                                                          \
    if (p.lpr == LPR_ && p.cpl == CPL_) {                                                                                          \
        note_kernel("attn_qkv_kernel<%s, %d, %d>", weight_type == WT_BF16 ? "unsigned short" : weight_type == WT_B24 ? "b24" : "float", \
                    LPR_, CPL_);                                                                                                   \
        if (weight_type == WT_BF16)                                                                                                \
            hipLaunchKernelGGL((attn_qkv_kernel<bf16_t, LPR_, CPL_>), dim3(grid), dim3(256), 0, s, g.W, g.x,                       \
                               (unsigned)g.N | ((unsigned)g.epilogue << 24), (unsigned)g.K | (G << 16), g.ln_g, g.ln_c2, g.ln_c3, cw, g, f); \
        else if (weight_type == WT_B24)                                                                                            \
            hipLaunchKernelGGL((attn_qkv_kernel<b24_t, LPR_, CPL_>), dim3(grid), dim3(256), 0, s, g.W, g.x,                        \
                               (unsigned)g.N | ((unsigned)g.epilogue << 24), (unsigned)g.K | (G << 16), g.ln_g, g.ln_c2, g.ln_c3, cw, g, f); \
        else                                                                                                                       \
            hipLaunchKernelGGL((attn_qkv_kernel<float, LPR_, CPL_>), dim3(grid), dim3(256), 0, s, g.W, g.x,                        \
                               (unsigned)g.N | ((unsigned)g.epilogue << 24), (unsigned)g.K | (G << 16), g.ln_g, g.ln_c2, g.ln_c3, cw, g, f); \
        ZG_HIP(hipGetLastError());                                                                                                 \
        return ZG_OK;                                                                                                              \
    }
    ZG_QA(16, 2)
    ZG_QA(32, 2)
    ZG_QA(32, 3)
    ZG_QA(64, 2)
#undef ZG_QA
    zg::set_error("fused c_attn + attention: no instantiation for K=%d", g.K);
    return ZG_ERR_UNSUPPORTED;
}

}  // namespace zg
