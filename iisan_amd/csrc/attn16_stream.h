// The chunk walk of the streaming-softmax attention kernels (device only), written once for the two head geometries:
//   attention16_long_kernel (attn16_long.hip: 64-wide heads, head-major input) and attention16_hd80_kernel (attn16_hd80.hip: 80-wide
//   heads, row-major input).  softmax(Q K^T / sqrt(head width) + key_bias) V with a working set that does not grow with S: a workgroup
//   owns one (item, head) and a set of 16-query blocks (grid.y), and walks the keys in chunks of 128:
//   * one chunk's K, V^T (permuted, as AttnLds<8> lays it out) and key limits sit in LDS; the next chunk's K / V pieces travel in registers
//     during the chunk's compute, as attention16_kernel prefetches the next head;
//   * a wave owns G::NQ query blocks and carries, for each, the running row maximum (already scaled by c2 = log2(e) / sqrt(head width)),
//     the running row sum and the f4 context accumulators; a chunk that raises the maximum rescales sum and context by exp2(ms_old - ms_new);
//   * per chunk and block the arithmetic is the shared one (attn16_block.h): transposed scores S^T = K Q^T, per-key limits, exp2 of one fma,
//     P rounded once to the operand type, O^T += V^T P^T, and attn_store_ctx at the end.
// What the rescale has to get right, and why it does (tests/test_gpu_attention_long.py, tests/test_gpu_vit_huge_attention.py):
//   * ms starts at -inf, and every chunk holds at least one key < S, whose limited score is >= MASK_RAW: ms_new is finite, exp2(-inf - ms_new)
//     = 0 and the first chunk starts from zeros without a special case;
//   * an entirely masked chunk behind real keys does not raise the maximum: p = exp2(MASK_RAW c2 - ms) = 0 for each of its keys;
//   * entirely masked chunks BEFORE the first real key leave ms = MASK_RAW c2 (exact: MASK_RAW is a power of two), p = 1 per key; the first
//     real key gives exp2(MASK_RAW c2 - ms_new) = 0 and their uniform contribution vanishes exactly;
//   * an all-masked item keeps ms = MASK_RAW c2 throughout: p = exp2(0) = 1 on its S keys, the result is the mean of V;
//   * structural pad slots of the last chunk (key >= S) are limited to -inf: p = 0; pad queries of the last block are never stored.
// The running maximum is kept SCALED (ms = max * c2, rounded once: the product with a positive constant is monotone, so max and scaling
// commute) so that the rescale exponent is a plain subtraction: no fma contraction can leave a rounding residue in exp2(ms - ms) = 1.
//
// A geometry G supplies what the head width and the input layout change, and nothing else:
//   HD, KSTEPS, DT          head width, 32-slot score steps per 16-key tile, 16-dim context tiles (64, 2, 4 | 80, 3, 5)
//   NQ, KBATCH              query blocks per wave; score tiles whose K fragments are requested together
//   C2                      log2(e) / sqrt(HD)
//   LDS, VT_OFF, KB_OFF     bytes of the chunk image, and where V^T and the key limits start in it
//   KPIECES                 16-byte K pieces per thread and chunk
//   q_base, plane, ld       element offset of the (item, head)'s Q; from Q to K and K to V; from one token's row to the next
//   qblock(i, wave)         the wave's i-th query block
//   k_piece, stage_k, k_off K piece p of a thread -> (row, 16-byte slot); its place in LDS; the LDS byte of the K fragment (row, step, g)
// What depends on HD > 64 (a third, half-empty score step; the V tail; the fifth context tile) is under `if constexpr` below.
#pragma once
#include "attn16_block.h"

constexpr int STREAM_NT = 8;                 // 16-key score tiles per chunk: 128 keys
constexpr int STREAM_CHUNK = STREAM_NT * 16;
constexpr int STREAM_MAX_S = 1024;

// grid = (items * heads, query ranges), 256 threads
template <typename T, class G>
__device__ __forceinline__ void attn_stream_body(const typename T::elem* __restrict__ qkv, const float* __restrict__ key_bias,
                                                 typename T::elem* __restrict__ ctx, int S, int heads) {
    typedef typename T::elem E;
    typedef typename T::v8 V8;
    typedef typename T::v4 V4;
    typedef AttnLds<STREAM_NT> L;        // V^T geometry (vt_at, vt_frag, stage_v_group, VT_LD) for both widths; K and the sizes are G's
    constexpr int HD = G::HD, NQ = G::NQ, DT = G::DT, KSTEPS = G::KSTEPS;
    constexpr bool WIDE = HD > 64;
    static_assert(L::VP == 1 && L::SP == STREAM_CHUNK, "one chunk = one V pass of 256 threads");
    static_assert(HD == 64 || HD == 80, "head dims past 64 are one 16-dim tile");
    __shared__ __attribute__((aligned(16))) char smem[G::LDS];
    char* sK = smem;
    E* sVt = (E*)(smem + G::VT_OFF);
    float* sKB = (float*)(smem + G::KB_OFF);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = blockIdx.x / heads, h = blockIdx.x - item * heads;
    const int D = heads * HD, ld = G::ld(D);
    const int j = lane & 15, g = lane >> 4;
    const int c = tid & 7, r0 = tid >> 3;
    // the 16 head dims past 64: 64 (four-key group, 8-dim piece) pairs per chunk, 16 lanes of every wave
    [[maybe_unused]] const bool vtail = lane < 16;
    [[maybe_unused]] const int kg1 = (wave * 16 + j) >> 1, c1 = 8 + (j & 1);
    const int nqb = (S + 15) >> 4, nch = (S + STREAM_CHUNK - 1) / STREAM_CHUNK;

    // 32-bit lane offsets from a uniform base
    const E* qb_ = qkv + G::q_base(item, h, S, heads, ld);
    const E* kb_ = qb_ + G::plane(S, D);
    const E* vb_ = kb_ + G::plane(S, D);

    // head dims 64..79 go through the same 32-slot MFMA step: lane groups 0 and 1 carry 8 dims each, groups 2 and 3 carry ZEROS in Q (what K
    // holds in their slots then does not matter, so K is read for them like for groups 0 and 1)
    V8 qf[NQ][KSTEPS];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        int sq = G::qblock(i, wave) * 16 + j;
        sq = sq < S ? sq : S - 1;                   // pad queries (and blocks past the last) re-read the last real row; never stored
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) qf[i][kk] = *(const V8*)(qb_ + (unsigned)(sq * ld + kk * 32 + g * 8));
        if constexpr (WIDE) {
            qf[i][2] = *(const V8*)(qb_ + (unsigned)(sq * ld + 64 + (g & 1) * 8));
            if (g >= 2) qf[i][2] = V8{};
        }
    }

    V8 kreg[G::KPIECES], vreg[4];
    [[maybe_unused]] V8 vreg1[4];
    float lim = 0.f;
    auto load_chunk = [&](int ch) {
        const int k0 = ch * STREAM_CHUNK;
#pragma unroll
        for (int p = 0; p < G::KPIECES; ++p) {
            int row, slot;
            G::k_piece(tid, p, row, slot);
            const int key = k0 + row;
            // pad slots (key >= S) re-read the last real row: their scores are forced to -inf by the key limit and their P is exactly 0.
            // (K / V are read once per query range, not once: no non-temporal hint here)
            kreg[p] = *(const V8*)(kb_ + (unsigned)((key < S ? key : S - 1) * ld + slot * 8));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + r0 * 4 + r;
            vreg[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * ld + c * 8));
        }
        if constexpr (WIDE) {
            if (vtail) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = k0 + kg1 * 4 + r;
                    vreg1[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * ld + c1 * 8));
                }
            }
        }
        if (tid < STREAM_CHUNK) lim = attn_key_limit(key_bias, item, S, k0 + tid);
    };

    float ms[NQ], sum[NQ];
    f4 o[NQ][DT];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        ms[i] = -INFINITY;
        sum[i] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[i][dt] = (f4){0.f, 0.f, 0.f, 0.f};
    }

    load_chunk(0);
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        if (ch > 0) __syncthreads();          // every wave is done reading the previous chunk's K / V^T / limits
#pragma unroll
        for (int p = 0; p < G::KPIECES; ++p) G::stage_k(sK, tid, p, kreg[p]);
        L::template stage_v_group<T>(sVt, tid, 0, vreg);
        if constexpr (WIDE) {
            if (vtail) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    V4 t;
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] = vreg1[r][e];
                    *(V4*)L::vt_at(sVt, c1 * 8 + e, kg1) = t;
                }
            }
        }
        if (tid < STREAM_CHUNK) sKB[tid] = lim;
        __syncthreads();
        if (ch + 1 < nch) load_chunk(ch + 1);   // in flight during this chunk's compute

#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int qb = G::qblock(i, wave);
            if (qb >= nqb) continue;             // wave-uniform

            // S^T tiles of the chunk: lane holds query j, keys k0 + 16 t + 4 g + r (raw dot products; the scale is folded into exp2)
            f4 sc[STREAM_NT];
            {
                constexpr int KBATCH = G::KBATCH;        // tiles whose K fragments are requested together
#pragma unroll
                for (int t0 = 0; t0 < STREAM_NT; t0 += KBATCH) {
                    V8 kf[KBATCH][KSTEPS];
#pragma unroll
                    for (int u = 0; u < KBATCH; ++u)
#pragma unroll
                        for (int kk = 0; kk < KSTEPS; ++kk) kf[u][kk] = *(const V8*)(sK + G::k_off((t0 + u) * 16 + j, kk, g));
#pragma unroll
                    for (int u = 0; u < KBATCH; ++u) {
                        f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int kk = 0; kk < KSTEPS; ++kk) acc = T::mfma(kf[u][kk], qf[i][kk], acc);
                        sc[t0 + u] = acc;
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < STREAM_NT; ++t) attn_apply_key_limit(sc[t], *(const f4*)(sKB + t * 16 + g * 4));
            const AttnChunkStat st = attn_chunk_softmax(sc, ms[i], G::C2);
            // rescale what the earlier chunks left (first chunk: exp2(-inf) = 0 on zeros; maximum not raised: exp2(0) = 1)
            const float alpha = __builtin_amdgcn_exp2f(ms[i] - st.ms);
            ms[i] = st.ms;
            sum[i] = sum[i] * alpha + st.sum;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[i][dt][r] *= alpha;
            // O^T += V^T · P^T: four 32-key steps over the 16-dim tiles
#pragma unroll
            for (int kb = 0; kb < STREAM_NT / 2; ++kb) {
                const V8 pf = attn_round_p<T>(sc[2 * kb], sc[2 * kb + 1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) o[i][dt] = T::mfma(L::template vt_frag<V8>(sVt, dt, j, g, kb), pf, o[i][dt]);
            }
        }
    }

#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int qb = G::qblock(i, wave);
        if (qb >= nqb) continue;
        const int sq = qb * 16 + j;
        const float inv = 1.0f / sum[i];
        E* base = ctx + (size_t)item * S * D;
        // head dims 0..63 in 16 contiguous bytes per lane (attn_store_ctx), 64..79 as the lane holds them (8 bytes)
        const f4 o4[4] = {o[i][0], o[i][1], o[i][2], o[i][3]};
        attn_store_ctx<T>(base, sq * D + h * HD, [&] { return g; }, o4, inv, sq < S);
        if constexpr (WIDE) {
            V4 ot;
#pragma unroll
            for (int r = 0; r < 4; ++r) ot[r] = T::from_f32(o[i][4][r] * inv);
            if (sq < S) *(V4*)(base + (unsigned)(sq * D + h * HD + 64 + g * 4)) = ot;
        }
    }
}

// The launcher of both kernels: `name` goes into the messages, `row` = the elements one token spans in the widest buffer the kernel
// addresses by 32-bit offsets (an item of S rows must stay below 2^31 elements), `count` is the file's dev counter.
template <class G, class K16, class KB16>
int launch_attn_stream(const char* name, K16 kernel_f16, KB16 kernel_bf16, int64_t row, int64_t& count, int dtype16, const void* qkv,
                       const float* key_bias, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    IISAN_CHECK_SHAPE(items > 0 && S > 0 && heads > 0, "%s: empty problem", name);
    IISAN_CHECK_SHAPE(S <= STREAM_MAX_S, "%s: sequence length %d > %d not supported", name, S, STREAM_MAX_S);
    IISAN_CHECK_SHAPE(items * heads < (1ll << 31), "%s: grid too large", name);
    IISAN_CHECK_SHAPE(S * row < (1ll << 31), "%s: item of %d x %d elements too large", name, S, (int)row);
    const int nqb = (S + 15) / 16;
    dim3 grid((unsigned)(items * heads), (unsigned)ceil_div(nqb, 4 * G::NQ)), block(256);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL(kernel_bf16, grid, block, 0, s, (const __bf16*)qkv, key_bias, (__bf16*)ctx, S, heads);
    else
        hipLaunchKernelGGL(kernel_f16, grid, block, 0, s, (const _Float16*)qkv, key_bias, (_Float16*)ctx, S, heads);
    IISAN_LAUNCH_OK();
    ++count;
    return IISAN_OK;
}
