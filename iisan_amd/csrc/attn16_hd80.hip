// Streaming-softmax attention for 80-wide heads (ViT-H/14: 16 heads x 80 = 1280): softmax(Q K^T / sqrt(80) + key_bias) V, 1 <= S <= 1,024.
// The chunk walk, the running-maximum rules and the per-block arithmetic are those of attention16_long_kernel (attn16_long.hip, whose
// header spells the rules out) and of attn16_block.h: MASK_RAW and the key limits, attn_chunk_softmax with c2 = log2(e) / sqrt(80), P
// rounded once, the V^T key permutation.  What the head width changes:
//   * INPUT: row-major [items * S, 3 * heads * 80], the output of a plain EPI_OUT16 product — Q, K, V of head h at columns h 80,
//     D + h 80, 2 D + h 80, a 160-byte run per token.  No GEMM epilogue knows the head width; the context goes out row-major as ever.
//   * Q K^T over K = 80: THREE v_mfma_f32_16x16x32 steps per 16-key tile — head dims 0..63 in two, and 64..79 in a third whose contraction
//     slots are half empty: lane groups 0 and 1 carry 8 dims each, groups 2 and 3 carry zeros in Q.  One opcode for the whole chain, not
//     two 32-slot steps + one 16x16x16 step (4 of 44 MFMA steps per block and chunk fewer): that chain gave scores that were right or
//     wrong by the instruction schedule on the MI355X (profiles/vit_huge.md §4; the supposed cause, not shown, is a wait state missing
//     between MFMAs of different pass counts), and this one does not depend on the schedule.
//   * P V over FIVE 16-dim output tiles: 20 context accumulators per query block; HD80_NQ = 3 blocks per wave (the long kernel: 4 x 16).
//   * LDS, one 128-key chunk, 44,032 B:
//       K   [128][80], rows of 160 bytes, NO padding and NO swizzle.  A ds_read_b128 is served in four groups of 16 lanes, each made of
//           eight lanes of lane group g (rows j in {0-3, 12-15} or {4-11}) and the other eight rows of lane group g + 1, one 16-byte slot
//           further (MI355X LDS table).  160 B = 10 bank quads: 10 j mod 16 over either row set is eight distinct values of ONE parity
//           ({0,10,4,14,8,2,12,6} / {8,2,12,6,0,10,4,14}), and the second half reads slot + 1, the other parity: 16 distinct bank
//           quads, conflict-free, for every slot pair of both 32-dim steps.  Tiles are 16 rows = 160 quads = 0 (mod 16) apart.
//           The third step reads slot 8 + (g & 1) — again slot and slot + 1 inside every group of 16 lanes: conflict-free.  Three
//           ds_read_b128 per tile and lane, 12 LDS cycles per wave and tile, 0 conflict cycles.
//           Staging is a straight copy: 16-byte piece p = tid + 256 i (i < 5) of the chunk is row p / 10, slot p % 10, LDS byte 16 p.
//       V^T [80][144] as AttnLds<8> lays it out (keys permuted inside groups of 32, row stride 288 B = 18 quads: 2 j for one half of
//           a group, 2 j + 1 for the other — conflict-free as for the 64-wide heads).  Head dims 0..63 are transposed by all 256 threads
//           (AttnLds::stage_v_group), dims 64..79 by 16 lanes of every wave.
//       per-key limits [128].
#include "attn16_block.h"

static int64_t g_attn16_hd80_count = 0;
IISAN_DEV_COUNTER(attn16_hd80, g_attn16_hd80_count);

namespace {

constexpr int HD = 80;
constexpr int HD80_NT = 8;               // 16-key score tiles per chunk: 128 keys
constexpr int HD80_CHUNK = HD80_NT * 16;
// Score tiles whose K fragments are requested together: 2 x 12 VGPRs.  (4, as in the long kernel, spills: 256 VGPRs + 60 B of scratch.)
#ifndef ATTN_HD80_KBATCH
#define ATTN_HD80_KBATCH 2
#endif
// 16-query blocks per wave.  Per block: Q 12 + context 20 + statistics 2 VGPRs; beside them one chunk's scores (32), the next chunk's K / V
// pieces (20 + 32) and the fragments.  3 keeps two waves per SIMD without scratch: 254 VGPRs, 0 B scratch, 44,032 B LDS (hipcc
// -Rpass-analysis=kernel-resource-usage; profiles/vit_huge.md); a workgroup covers 192 queries of its (item, head) per chunk it stages.
#ifndef ATTN_HD80_NQ
#define ATTN_HD80_NQ 3
#endif
constexpr int HD80_NQ = ATTN_HD80_NQ;
constexpr int HD80_MAX_S = 1024;
// exp(s / sqrt(80) - m) = exp2(acc * c2 - m2),  c2 = log2(e) / sqrt(80)
constexpr float HD80_C2 = 0.16129820911147802f;

constexpr int HD80_KROW = HD * 2;                                        // bytes of a K row in LDS
constexpr int HD80_KPIECES = HD80_CHUNK * HD / 8 / 256;                  // 16-byte K pieces per thread and chunk: 5
constexpr int HD80_VT_OFF = HD80_CHUNK * HD80_KROW;                      // 20,480
constexpr int HD80_KB_OFF = HD80_VT_OFF + HD * AttnLds<HD80_NT>::VT_LD * 2;   // + 23,040
constexpr int HD80_LDS = HD80_KB_OFF + HD80_CHUNK * 4;                   // 44,032
static_assert(HD80_KPIECES * 256 * 8 == HD80_CHUNK * HD, "the K pieces of a chunk divide evenly over 256 threads");

// grid = (items * heads, query ranges), 256 threads.  Query block (i gridDim.y + blockIdx.y) 4 + wave is block i of a wave: the ranges
// interleave, so the last, partial range of blocks is spread over the workgroups of a head instead of left to one of them.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention16_hd80_kernel(const typename T::elem* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                  typename T::elem* __restrict__ ctx, int S, int heads) {
    typedef typename T::elem E;
    typedef typename T::v8 V8;
    typedef typename T::v4 V4;
    typedef AttnLds<HD80_NT> L;          // V^T geometry only (vt_at, vt_frag, stage_v_group, VT_LD); K and the sizes are this file's
    __shared__ __attribute__((aligned(16))) char smem[HD80_LDS];
    char* sK = smem;
    E* sVt = (E*)(smem + HD80_VT_OFF);
    float* sKB = (float*)(smem + HD80_KB_OFF);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = blockIdx.x / heads, h = blockIdx.x - item * heads;
    const int D = heads * HD, ld = 3 * D;
    const int j = lane & 15, g = lane >> 4;
    const int c = tid & 7, r0 = tid >> 3;
    // the 16 head dims past 64: 64 (four-key group, 8-dim piece) pairs per chunk, 16 lanes of every wave
    const bool vtail = lane < 16;
    const int kg1 = (wave * 16 + j) >> 1, c1 = 8 + (j & 1);
    const int nqb = (S + 15) >> 4, nch = (S + HD80_CHUNK - 1) / HD80_CHUNK;

    // row-major input: token row (item S + s), columns [q | k | v] x [head] x 80; 32-bit lane offsets from a uniform base
    const E* qb_ = qkv + (int64_t)item * S * ld + h * HD;
    const E* kb_ = qb_ + D;
    const E* vb_ = kb_ + D;

    // head dims 64..79 go through the same 32-slot MFMA step: lane groups 0 and 1 carry 8 dims each, groups 2 and 3 carry ZEROS in Q (what K
    // holds in their slots then does not matter, so K is read for them like for groups 0 and 1)
    V8 qf[HD80_NQ][3];
#pragma unroll
    for (int i = 0; i < HD80_NQ; ++i) {
        int sq = ((i * gridDim.y + blockIdx.y) * 4 + wave) * 16 + j;
        sq = sq < S ? sq : S - 1;                   // pad queries (and blocks past the last) re-read the last real row; never stored
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[i][kk] = *(const V8*)(qb_ + (unsigned)(sq * ld + kk * 32 + g * 8));
        qf[i][2] = *(const V8*)(qb_ + (unsigned)(sq * ld + 64 + (g & 1) * 8));
        if (g >= 2) qf[i][2] = V8{};
    }

    V8 kreg[HD80_KPIECES], vreg[4], vreg1[4];
    float lim = 0.f;
    auto load_chunk = [&](int ch) {
        const int k0 = ch * HD80_CHUNK;
#pragma unroll
        for (int p = 0; p < HD80_KPIECES; ++p) {
            const int piece = tid + 256 * p, row = piece / 10, slot = piece - row * 10;
            const int key = k0 + row;
            // pad slots (key >= S) re-read the last real row: their scores are forced to -inf by the key limit and their P is exactly 0
            kreg[p] = *(const V8*)(kb_ + (unsigned)((key < S ? key : S - 1) * ld + slot * 8));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + r0 * 4 + r;
            vreg[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * ld + c * 8));
        }
        if (vtail) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + kg1 * 4 + r;
                vreg1[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * ld + c1 * 8));
            }
        }
        if (tid < HD80_CHUNK) lim = attn_key_limit(key_bias, item, S, k0 + tid);
    };

    float ms[HD80_NQ], sum[HD80_NQ];
    f4 o[HD80_NQ][5];
#pragma unroll
    for (int i = 0; i < HD80_NQ; ++i) {
        ms[i] = -INFINITY;
        sum[i] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 5; ++dt) o[i][dt] = (f4){0.f, 0.f, 0.f, 0.f};
    }

    load_chunk(0);
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        if (ch > 0) __syncthreads();          // every wave is done reading the previous chunk's K / V^T / limits
#pragma unroll
        for (int p = 0; p < HD80_KPIECES; ++p) *(V8*)(sK + (tid + 256 * p) * 16) = kreg[p];
        L::template stage_v_group<T>(sVt, tid, 0, vreg);
        if (vtail) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                V4 t;
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] = vreg1[r][e];
                *(V4*)L::vt_at(sVt, c1 * 8 + e, kg1) = t;
            }
        }
        if (tid < HD80_CHUNK) sKB[tid] = lim;
        __syncthreads();
        if (ch + 1 < nch) load_chunk(ch + 1);   // in flight during this chunk's compute

#pragma unroll
        for (int i = 0; i < HD80_NQ; ++i) {
            const int qb = (i * gridDim.y + blockIdx.y) * 4 + wave;
            if (qb >= nqb) continue;             // wave-uniform

            // S^T tiles of the chunk: lane holds query j, keys k0 + 16 t + 4 g + r (raw dot products; the scale is folded into exp2)
            f4 sc[HD80_NT];
            {
                constexpr int KBATCH = ATTN_HD80_KBATCH;        // tiles whose K fragments are requested together
#pragma unroll
                for (int t0 = 0; t0 < HD80_NT; t0 += KBATCH) {
                    V8 kf[KBATCH][3];
#pragma unroll
                    for (int u = 0; u < KBATCH; ++u) {
                        const char* row = sK + ((t0 + u) * 16 + j) * HD80_KROW;
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk) kf[u][kk] = *(const V8*)(row + (kk * 4 + g) * 16);
                        kf[u][2] = *(const V8*)(row + (8 + (g & 1)) * 16);
                    }
#pragma unroll
                    for (int u = 0; u < KBATCH; ++u) {
                        f4 acc = {0.f, 0.f, 0.f, 0.f};
                        acc = T::mfma(kf[u][0], qf[i][0], acc);
                        acc = T::mfma(kf[u][1], qf[i][1], acc);
                        sc[t0 + u] = T::mfma(kf[u][2], qf[i][2], acc);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < HD80_NT; ++t) attn_apply_key_limit(sc[t], *(const f4*)(sKB + t * 16 + g * 4));
            const AttnChunkStat st = attn_chunk_softmax(sc, ms[i], HD80_C2);
            // rescale what the earlier chunks left (first chunk: exp2(-inf) = 0 on zeros; maximum not raised: exp2(0) = 1)
            const float alpha = __builtin_amdgcn_exp2f(ms[i] - st.ms);
            ms[i] = st.ms;
            sum[i] = sum[i] * alpha + st.sum;
#pragma unroll
            for (int dt = 0; dt < 5; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[i][dt][r] *= alpha;
            // O^T += V^T · P^T: four 32-key steps over five 16-dim tiles
#pragma unroll
            for (int kb = 0; kb < HD80_NT / 2; ++kb) {
                const V8 pf = attn_round_p<T>(sc[2 * kb], sc[2 * kb + 1]);
#pragma unroll
                for (int dt = 0; dt < 5; ++dt) o[i][dt] = T::mfma(L::template vt_frag<V8>(sVt, dt, j, g, kb), pf, o[i][dt]);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < HD80_NQ; ++i) {
        const int qb = (i * gridDim.y + blockIdx.y) * 4 + wave;
        if (qb >= nqb) continue;
        const int sq = qb * 16 + j;
        const float inv = 1.0f / sum[i];
        E* base = ctx + (size_t)item * S * D;
        // head dims 0..63 as the 64-wide kernels store them (16 contiguous bytes per lane), 64..79 as the lane holds them (8 bytes)
        const f4 o4[4] = {o[i][0], o[i][1], o[i][2], o[i][3]};
        attn_store_ctx<T>(base, sq * D + h * HD, [&] { return g; }, o4, inv, sq < S);
        V4 ot;
#pragma unroll
        for (int r = 0; r < 4; ++r) ot[r] = T::from_f32(o[i][4][r] * inv);
        if (sq < S) *(V4*)(base + (unsigned)(sq * D + h * HD + 64 + g * 4)) = ot;
    }
}

}  // namespace

int launch_attention16_hd80(int dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    IISAN_CHECK_SHAPE(items > 0 && S > 0 && heads > 0, "attention16_hd80: empty problem");
    IISAN_CHECK_SHAPE(S <= HD80_MAX_S, "attention16_hd80: sequence length %d > %d not supported", S, HD80_MAX_S);
    IISAN_CHECK_SHAPE(items * heads < (1ll << 31), "attention16_hd80: grid too large");
    IISAN_CHECK_SHAPE((int64_t)S * heads * HD * 3 < (1ll << 31), "attention16_hd80: item of %d x %d elements too large", S, heads * HD * 3);
    const int nqb = (S + 15) / 16;
    dim3 grid((unsigned)(items * heads), (unsigned)ceil_div(nqb, 4 * HD80_NQ)), block(256);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL(attention16_hd80_kernel<BF16>, grid, block, 0, s, (const __bf16*)qkv, key_bias, (__bf16*)ctx, S, heads);
    else
        hipLaunchKernelGGL(attention16_hd80_kernel<F16>, grid, block, 0, s, (const _Float16*)qkv, key_bias, (_Float16*)ctx, S, heads);
    IISAN_LAUNCH_OK();
    ++g_attn16_hd80_count;
    return IISAN_OK;
}

extern "C" int iisan_attention16_hd80(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                                      int32_t heads, void* stream) {
    return launch_attention16_hd80(dtype16, qkv, key_bias, ctx, items, S, heads, (hipStream_t)stream);
}
