// Streaming-softmax attention for 80-wide heads (ViT-H/14: 16 heads x 80 = 1280): softmax(Q K^T / sqrt(80) + key_bias) V, 1 <= S <= 1,024.
// The chunk walk, the running-maximum rules and what the rescale has to get right are attn16_stream.h's, shared with the 64-wide heads
// (attn16_long.hip); the per-block arithmetic is attn16_block.h's: MASK_RAW and the key limits, attn_chunk_softmax with c2 = log2(e) /
// sqrt(80), P rounded once, the V^T key permutation.  This file is the geometry of an 80-wide head.  What the head width changes:
//   * INPUT: row-major [items * S, 3 * heads * 80], the output of a plain EPI_OUT16 product — Q, K, V of head h at columns h 80,
//     D + h 80, 2 D + h 80, a 160-byte run per token.  No GEMM epilogue knows the head width; the context goes out row-major as ever.
//   * Q K^T over K = 80: THREE v_mfma_f32_16x16x32 steps per 16-key tile — head dims 0..63 in two, and 64..79 in a third whose contraction
//     slots are half empty: lane groups 0 and 1 carry 8 dims each, groups 2 and 3 carry zeros in Q.  One opcode for the whole chain, not
//     two 32-slot steps + one 16x16x16 step (4 of 44 MFMA steps per block and chunk fewer): that chain gave scores that were right or
//     wrong by the instruction schedule on the MI355X (profiles/vit_huge.md §4; the supposed cause, not shown, is a wait state missing
//     between MFMAs of different pass counts), and this one does not depend on the schedule.
//   * P V over FIVE 16-dim output tiles: 20 context accumulators per query block; ATTN_HD80_NQ = 3 blocks per wave (the long kernel: 4 x 16).
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
#include "attn16_stream.h"

static int64_t g_attn16_hd80_count = 0;
IISAN_DEV_COUNTER(attn16_hd80, g_attn16_hd80_count);

namespace {

// Score tiles whose K fragments are requested together: 2 x 12 VGPRs.  (4, as in the long kernel, spills: 256 VGPRs + 60 B of scratch.)
#ifndef ATTN_HD80_KBATCH
#define ATTN_HD80_KBATCH 2
#endif
// 16-query blocks per wave.  Per block: Q 12 + context 20 + statistics 2 VGPRs; beside them one chunk's scores (32), the next chunk's K / V
// pieces (20 + 32) and the fragments.  3 keeps two waves per SIMD without scratch: 255 VGPRs, 0 B scratch, 44,032 B LDS (hipcc
// -Rpass-analysis=kernel-resource-usage; profiles/vit_huge.md); a workgroup covers 192 queries of its (item, head) per chunk it stages.
#ifndef ATTN_HD80_NQ
#define ATTN_HD80_NQ 3
#endif

struct Hd80Geom {
    static constexpr int HD = 80, KSTEPS = 3, DT = 5, NQ = ATTN_HD80_NQ, KBATCH = ATTN_HD80_KBATCH;
    // exp(s / sqrt(80) - m) = exp2(acc * c2 - m2),  c2 = log2(e) / sqrt(80)
    static constexpr float C2 = 0.16129820911147802f;
    static constexpr int KROW = HD * 2;                                          // bytes of a K row in LDS
    static constexpr int KPIECES = STREAM_CHUNK * HD / 8 / 256;                  // 16-byte K pieces per thread and chunk: 5
    static constexpr int VT_OFF = STREAM_CHUNK * KROW;                           // 20,480
    static constexpr int KB_OFF = VT_OFF + HD * AttnLds<STREAM_NT>::VT_LD * 2;   // + 23,040
    static constexpr int LDS = KB_OFF + STREAM_CHUNK * 4;                        // 44,032
    static_assert(KPIECES * 256 * 8 == STREAM_CHUNK * HD, "the K pieces of a chunk divide evenly over 256 threads");
    // row-major input: token row (item S + s), columns [q | k | v] x [head] x 80
    static __device__ __forceinline__ int64_t q_base(int item, int h, int S, int, int ld) { return (int64_t)item * S * ld + h * HD; }
    static __device__ __forceinline__ int plane(int, int D) { return D; }
    static __device__ __forceinline__ int ld(int D) { return 3 * D; }
    // Query block (i gridDim.y + blockIdx.y) 4 + wave is block i of a wave: the ranges interleave, so the last, partial range of blocks is
    // spread over the workgroups of a head instead of left to one of them.
    static __device__ __forceinline__ unsigned qblock(int i, int wave) { return (i * gridDim.y + blockIdx.y) * 4 + wave; }
    static __device__ __forceinline__ void k_piece(int tid, int p, int& row, int& slot) {
        const int piece = tid + 256 * p;
        row = piece / 10, slot = piece - row * 10;
    }
    template <class V8>
    static __device__ __forceinline__ void stage_k(char* sK, int tid, int p, const V8& k) { *(V8*)(sK + (tid + 256 * p) * 16) = k; }
    static __device__ __forceinline__ int k_off(int row, int step, int g) { return row * KROW + (step < 2 ? step * 4 + g : 8 + (g & 1)) * 16; }
};

template <typename T>
__global__ __launch_bounds__(256, 2) void attention16_hd80_kernel(const typename T::elem* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                  typename T::elem* __restrict__ ctx, int S, int heads) {
    attn_stream_body<T, Hd80Geom>(qkv, key_bias, ctx, S, heads);
}

}  // namespace

int launch_attention16_hd80(int dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    return launch_attn_stream<Hd80Geom>("attention16_hd80", attention16_hd80_kernel<F16>, attention16_hd80_kernel<BF16>,
                                        (int64_t)heads * Hd80Geom::HD * 3, g_attn16_hd80_count, dtype16, qkv, key_bias, ctx, items, S, heads, s);
}

extern "C" int iisan_attention16_hd80(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                                      int32_t heads, void* stream) {
    return launch_attention16_hd80(dtype16, qkv, key_bias, ctx, items, S, heads, (hipStream_t)stream);
}
