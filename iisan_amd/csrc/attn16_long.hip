// Streaming-softmax attention of the frozen encoders for sequences past 224 tokens (head_dim 64): softmax(Q K^T / 8 + key_bias) V with a
// working set that does not grow with S.  attention16_kernel (attn16.hip) keeps a whole head's K and V^T in LDS and one query row's scores
// in registers; here a workgroup owns one (item, head) and a RANGE of 16-query blocks (grid.y), and walks the keys in chunks of 128:
//   * one chunk's K (swizzled) and V^T (permuted) sit in LDS as AttnLds<8> lays them out — 35,328 B with the chunk's key limits; the next
//     chunk's K / V rows travel in registers during the chunk's compute, as attention16_kernel prefetches the next head;
//   * a wave owns LONG_NQ query blocks of the range (block (y LONG_NQ + i) 4 + wave) and carries, for each, the running row maximum (already
//     scaled by c2 = log2(e) / 8), the running row sum and the four f4 context accumulators; a chunk that raises the maximum rescales sum and
//     context by exp2(ms_old - ms_new);
//   * per chunk and block the arithmetic is the shared one (attn16_block.h): transposed scores S^T = K Q^T, per-key limits, exp2 of one fma,
//     P rounded once to the operand type, O^T += V^T P^T, and attn_store_ctx at the end.
// What the rescale has to get right, and why it does (tests/test_gpu_attention_long.py):
//   * ms starts at -inf, and every chunk holds at least one key < S, whose limited score is >= MASK_RAW: ms_new is finite, exp2(-inf - ms_new)
//     = 0 and the first chunk starts from zeros without a special case;
//   * an entirely masked chunk behind real keys does not raise the maximum: p = exp2(MASK_RAW c2 - ms) = 0 for each of its keys;
//   * entirely masked chunks BEFORE the first real key leave ms = MASK_RAW c2 (exact: MASK_RAW is a power of two), p = 1 per key; the first
//     real key gives exp2(MASK_RAW c2 - ms_new) = 0 and their uniform contribution vanishes exactly;
//   * an all-masked item keeps ms = MASK_RAW c2 throughout: p = exp2(0) = 1 on its S keys, the result is the mean of V;
//   * structural pad slots of the last chunk (key >= S) are limited to -inf: p = 0; pad queries of the last block are never stored.
// The running maximum is kept SCALED (ms = max * c2, rounded once: the product with a positive constant is monotone, so max and scaling
// commute) so that the rescale exponent is a plain subtraction: no fma contraction can leave a rounding residue in exp2(ms - ms) = 1.
#include "attn16_block.h"

static int64_t g_attn16_long_count = 0;
IISAN_DEV_COUNTER(attn16_long, g_attn16_long_count);

namespace {

constexpr int LONG_NT = 8;               // 16-key score tiles per chunk: 128 keys
constexpr int LONG_CHUNK = LONG_NT * 16;
// 16-query blocks per wave: a workgroup covers 4 * LONG_NQ * 16 = 256 queries of its (item, head) and stages every chunk once for them.
// Measured at 128 items x 12 heads (tools/attn_long_time.py, variant builds with -DATTN_LONG_NQ, same run): 1 / 2 / 3 / 4 blocks per wave
// = 1,343 / 1,041 / 935 / 844 us at S = 1,024 and 481 / 439 / 402 / 381 us at S = 577 (profiles/long_sequences.md); 4 is 222 VGPRs, the
// last count that keeps two waves per SIMD without scratch.
#ifndef ATTN_LONG_NQ
#define ATTN_LONG_NQ 4
#endif
constexpr int LONG_NQ = ATTN_LONG_NQ;
constexpr int LONG_MAX_S = 1024;

// grid = (items * heads, query ranges), 256 threads.  Registers: 4 x (Q 8 + context 16 + statistics 2) per wave's blocks, one chunk's scores
// (32), the next chunk's K / V rows (32), K / V^T fragments: 222 VGPRs, no scratch (tests/test_isa_long_attention.py); LDS 35,328 B.
template <typename T>
__global__ __launch_bounds__(256, 2) void attention16_long_kernel(const typename T::elem* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                  typename T::elem* __restrict__ ctx, int S, int heads) {
    typedef typename T::elem E;
    typedef typename T::v8 V8;
    typedef AttnLds<LONG_NT> L;
    constexpr int KP = L::KP;            // 4 K passes of 32 rows; one V pass of 32 four-key groups
    static_assert(L::VP == 1 && L::SP == LONG_CHUNK, "one chunk = one V pass of 256 threads");
    __shared__ __attribute__((aligned(16))) char smem[L::BYTES];
    char* sK = smem;
    E* sVt = (E*)(smem + L::VT_OFF);
    float* sKB = (float*)(smem + L::KB_OFF);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = blockIdx.x / heads, h = blockIdx.x - item * heads;
    const int D = heads * 64;
    const int j = lane & 15, g = lane >> 4;
    const int c = tid & 7, r0 = tid >> 3;
    const int nqb = (S + 15) >> 4, nch = (S + LONG_CHUNK - 1) / LONG_CHUNK;

    // head-major input [item][head][q|k|v][S][64]: three contiguous blocks per (item, head); 32-bit lane offsets from a uniform base
    const E* qb_ = qkv + ((int64_t)item * heads + h) * 3 * S * 64;
    const E* kb_ = qb_ + (int64_t)S * 64;
    const E* vb_ = kb_ + (int64_t)S * 64;

    V8 qf[LONG_NQ][2];
#pragma unroll
    for (int i = 0; i < LONG_NQ; ++i) {
        int sq = ((blockIdx.y * LONG_NQ + i) * 4 + wave) * 16 + j;
        sq = sq < S ? sq : S - 1;                   // pad queries (and blocks past the last) re-read the last real row; never stored
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[i][kk] = *(const V8*)(qb_ + (unsigned)(sq * 64 + kk * 32 + g * 8));
    }

    V8 kreg[KP], vreg[4];
    float lim = 0.f;
    auto load_chunk = [&](int ch) {
        const int k0 = ch * LONG_CHUNK;
#pragma unroll
        for (int p = 0; p < KP; ++p) {
            const int key = k0 + r0 + 32 * p;
            // pad slots (key >= S) re-read the last real row: their scores are forced to -inf by the key limit and their P is exactly 0.
            // (K / V are read once per query range, not once: no non-temporal hint here)
            kreg[p] = *(const V8*)(kb_ + (unsigned)((key < S ? key : S - 1) * 64 + c * 8));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + r0 * 4 + r;
            vreg[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * 64 + c * 8));
        }
        if (tid < LONG_CHUNK) lim = attn_key_limit(key_bias, item, S, k0 + tid);
    };

    float ms[LONG_NQ], sum[LONG_NQ];
    f4 o[LONG_NQ][4];
#pragma unroll
    for (int i = 0; i < LONG_NQ; ++i) {
        ms[i] = -INFINITY;
        sum[i] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[i][dt] = (f4){0.f, 0.f, 0.f, 0.f};
    }

    load_chunk(0);
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        if (ch > 0) __syncthreads();          // every wave is done reading the previous chunk's K / V^T / limits
#pragma unroll
        for (int p = 0; p < KP; ++p) L::stage_k_row(sK, r0 + 32 * p, c, kreg[p]);
        L::template stage_v_group<T>(sVt, tid, 0, vreg);
        if (tid < LONG_CHUNK) sKB[tid] = lim;
        __syncthreads();
        if (ch + 1 < nch) load_chunk(ch + 1);   // in flight during this chunk's compute

#pragma unroll
        for (int i = 0; i < LONG_NQ; ++i) {
            const int qb = (blockIdx.y * LONG_NQ + i) * 4 + wave;
            if (qb >= nqb) continue;             // wave-uniform

            // S^T tiles of the chunk: lane holds query j, keys k0 + 16 t + 4 g + r (raw dot products; the 1/8 scale is folded into exp2)
            f4 sc[LONG_NT];
            {
                constexpr int KBATCH = 4;        // tiles whose K fragments are requested together
#pragma unroll
                for (int t0 = 0; t0 < LONG_NT; t0 += KBATCH) {
                    V8 kf[KBATCH][2];
#pragma unroll
                    for (int u = 0; u < KBATCH; ++u)
#pragma unroll
                        for (int kk = 0; kk < 2; ++kk) kf[u][kk] = *(const V8*)(sK + L::k_off((t0 + u) * 16 + j, kk * 4 + g));
#pragma unroll
                    for (int u = 0; u < KBATCH; ++u) {
                        f4 acc = {0.f, 0.f, 0.f, 0.f};
                        acc = T::mfma(kf[u][0], qf[i][0], acc);
                        acc = T::mfma(kf[u][1], qf[i][1], acc);
                        sc[t0 + u] = acc;
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < LONG_NT; ++t) attn_apply_key_limit(sc[t], *(const f4*)(sKB + t * 16 + g * 4));
            const AttnChunkStat st = attn_chunk_softmax(sc, ms[i]);
            // rescale what the earlier chunks left (first chunk: exp2(-inf) = 0 on zeros; maximum not raised: exp2(0) = 1)
            const float alpha = __builtin_amdgcn_exp2f(ms[i] - st.ms);
            ms[i] = st.ms;
            sum[i] = sum[i] * alpha + st.sum;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[i][dt][r] *= alpha;
            // O^T += V^T · P^T: four 32-key steps
#pragma unroll
            for (int kb = 0; kb < LONG_NT / 2; ++kb) {
                const V8 pf = attn_round_p<T>(sc[2 * kb], sc[2 * kb + 1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[i][dt] = T::mfma(L::template vt_frag<V8>(sVt, dt, j, g, kb), pf, o[i][dt]);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < LONG_NQ; ++i) {
        const int qb = (blockIdx.y * LONG_NQ + i) * 4 + wave;
        if (qb >= nqb) continue;
        const int sq = qb * 16 + j;
        attn_store_ctx<T>(ctx + (size_t)item * S * D, sq * D + h * 64, [&] { return g; }, o[i], 1.0f / sum[i], sq < S);
    }
}

}  // namespace

int launch_attention16_long(int dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    IISAN_CHECK_SHAPE(items > 0 && S > 0 && heads > 0, "attention16_long: empty problem");
    IISAN_CHECK_SHAPE(S <= LONG_MAX_S, "attention16_long: sequence length %d > %d not supported", S, LONG_MAX_S);
    IISAN_CHECK_SHAPE(items * heads < (1ll << 31), "attention16_long: grid too large");
    IISAN_CHECK_SHAPE((int64_t)S * heads * 64 < (1ll << 31), "attention16_long: item of %d x %d elements too large", S, heads * 64);
    const int nqb = (S + 15) / 16;
    dim3 grid((unsigned)(items * heads), (unsigned)ceil_div(nqb, 4 * LONG_NQ)), block(256);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL(attention16_long_kernel<BF16>, grid, block, 0, s, (const __bf16*)qkv, key_bias, (__bf16*)ctx, S, heads);
    else
        hipLaunchKernelGGL(attention16_long_kernel<F16>, grid, block, 0, s, (const _Float16*)qkv, key_bias, (_Float16*)ctx, S, heads);
    IISAN_LAUNCH_OK();
    ++g_attn16_long_count;
    return IISAN_OK;
}

extern "C" int iisan_attention16_long(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                                      int32_t heads, void* stream) {
    return launch_attention16_long(dtype16, qkv, key_bias, ctx, items, S, heads, (hipStream_t)stream);
}
