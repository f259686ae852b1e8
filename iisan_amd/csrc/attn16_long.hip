// Streaming-softmax attention of the frozen encoders for sequences past 224 tokens (head_dim 64): softmax(Q K^T / 8 + key_bias) V with a
// working set that does not grow with S.  attention16_kernel (attn16.hip) keeps a whole head's K and V^T in LDS and one query row's scores
// in registers; here a workgroup owns one (item, head) and a RANGE of 16-query blocks (grid.y), and walks the keys in chunks of 128.  The
// chunk walk, the running-maximum rules and what the rescale has to get right are attn16_stream.h's, shared with the 80-wide heads
// (attn16_hd80.hip); this file is the geometry of a 64-wide head:
//   * input head-major [item][head][q|k|v][S][64], three contiguous blocks per (item, head), as the QKV epilogue of the encoders writes it;
//   * one chunk's K (swizzled) and V^T (permuted) sit in LDS as AttnLds<8> lays them out — 35,328 B with the chunk's key limits;
//   * a wave owns ATTN_LONG_NQ CONTIGUOUS query blocks of the workgroup's range: block (y ATTN_LONG_NQ + i) 4 + wave.
#include "attn16_stream.h"

static int64_t g_attn16_long_count = 0;
IISAN_DEV_COUNTER(attn16_long, g_attn16_long_count);

namespace {

// 16-query blocks per wave: a workgroup covers 4 * ATTN_LONG_NQ * 16 = 256 queries of its (item, head) and stages every chunk once for them.
// Measured at 128 items x 12 heads (tools/attn_long_time.py, variant builds with -DATTN_LONG_NQ, same run): 1 / 2 / 3 / 4 blocks per wave
// = 1,343 / 1,041 / 935 / 844 us at S = 1,024 and 481 / 439 / 402 / 381 us at S = 577 (profiles/long_sequences.md); 4 is 222 VGPRs, the
// last count that keeps two waves per SIMD without scratch.
#ifndef ATTN_LONG_NQ
#define ATTN_LONG_NQ 4
#endif

struct LongGeom {
    typedef AttnLds<STREAM_NT> L;
    static constexpr int HD = 64, KSTEPS = 2, DT = 4, NQ = ATTN_LONG_NQ, KBATCH = 4;
    static constexpr float C2 = ATTN_C2;
    static constexpr int LDS = L::BYTES, VT_OFF = L::VT_OFF, KB_OFF = L::KB_OFF;
    static constexpr int KPIECES = L::KP;            // 4 K passes of 32 rows
    static __device__ __forceinline__ int64_t q_base(int item, int h, int S, int heads, int) { return ((int64_t)item * heads + h) * 3 * S * 64; }
    static __device__ __forceinline__ int64_t plane(int S, int) { return (int64_t)S * 64; }
    static __device__ __forceinline__ int ld(int) { return 64; }
    static __device__ __forceinline__ unsigned qblock(int i, int wave) { return (blockIdx.y * NQ + i) * 4 + wave; }
    static __device__ __forceinline__ void k_piece(int tid, int p, int& row, int& slot) { row = (tid >> 3) + 32 * p, slot = tid & 7; }
    template <class V8>
    static __device__ __forceinline__ void stage_k(char* sK, int tid, int p, const V8& k) { L::stage_k_row(sK, (tid >> 3) + 32 * p, tid & 7, k); }
    static __device__ __forceinline__ int k_off(int row, int step, int g) { return L::k_off(row, 4 * step + g); }
};

// Registers: 4 x (Q 8 + context 16 + statistics 2) per wave's blocks, one chunk's scores (32), the next chunk's K / V rows (32), K / V^T
// fragments: 222 VGPRs, no scratch (tests/test_isa_long_attention.py); LDS 35,328 B.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention16_long_kernel(const typename T::elem* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                  typename T::elem* __restrict__ ctx, int S, int heads) {
    attn_stream_body<T, LongGeom>(qkv, key_bias, ctx, S, heads);
}

}  // namespace

int launch_attention16_long(int dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    return launch_attn_stream<LongGeom>("attention16_long", attention16_long_kernel<F16>, attention16_long_kernel<BF16>, (int64_t)heads * 64,
                                        g_attn16_long_count, dtype16, qkv, key_bias, ctx, items, S, heads, s);
}

extern "C" int iisan_attention16_long(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                                      int32_t heads, void* stream) {
    return launch_attention16_long(dtype16, qkv, key_bias, ctx, items, S, heads, (hipStream_t)stream);
}
