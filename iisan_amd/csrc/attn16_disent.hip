// Disentangled self-attention of DeBERTa-v2/v3 (HF modeling_deberta_v2.py, DisentangledSelfAttention with share_att_key and
// pos_att_type = c2p | p2c), head_dim 64, for titles of up to 128 words:
//     score[i][j] = (Q_i . K_j  +  Q_i . PK[d]  +  K_j . PQ[d]) / sqrt(3 * 64) + key_bias[j],      d = i - j + span
//     ctx = softmax_j(score) V
// PK / PQ are the layer's projected position tables (iisan_deberta_rel_project: [heads][3][2 span][64], third 0 = PQ, third 1 = PK).  HF maps
// i - j through log buckets; that map is the identity for |i - j| <= span / 2, and the executor refuses longer titles, so d is used as it is.
// Input and output as attention16_kernel (attn16.hip): head-major qkv [item][head][q|k|v][S][64], token-major ctx.
//
// One (item, head) = one LDS image: K (swizzled rows) and V^T exactly as AttnLds lays them out, + the table rows the head can touch.  Local
// table row w of the image <-> d = w - SP + span (SP = 16 NT16, the padded length), so the pair (i, j) reads local row i - j + SP: rows
// 1 .. 2 SP - 1, and a title of S <= span words reaches d = 1 .. 2 span - 1 only.  Rows outside the table (reached by pad keys / pad queries alone:
// their scores are removed by the key limit, their context rows are not stored) are clamped re-reads of a real row.
// At NT16 = 8 (S = 128): K 16 KiB + V^T 18 KiB + 2 x 32 KiB of table rows + 19 KiB of diagonal scratch = 118 KiB of dynamic LDS.
//
// Per 16-query x 16-key block (qb, t) of a wave, on v_mfma_f32_16x16x32 (scores transposed as in attn16_block.h: a lane (j = lane & 15,
// g = lane >> 4) holds query j, keys 16 t + 4 g + r):
//   * S^T  = K_t . Q^T                                                   (2 MFMAs)
//   * the block's pairs cover i - j = 16 (qb - t) - 15 .. + 15: a WINDOW of 32 local table rows from w0 = 16 (qb - t) - 16 + SP on
//     (row w0 + wl, wl = j - kk + 16 in 1 .. 31, for query j and key kk of the block);
//   * C1 = PK[window] . Q^T   (A = 32 window rows in two tiles, B = the Q fragments: lane (j, g) holds window rows 16 u + 4 g + r of query j)
//   * C2 = PQ[window] . K_t^T (A = the same rows of PQ, B = the K fragments — an A fragment of K is also its B fragment: lane (kk, g) holds
//     window rows 16 u + 4 g + r of key kk)                                                              (4 + 4 MFMAs: 5 x the score work)
//   * the two blocks go to the wave's own LDS scratch and come back along their DIAGONALS: lane (j, g) register r (key kk = 4 g + r) reads
//     C1[wl][j] and C2[kk][wl].  ds_read_b32 / ds_write_b32 serve lanes 0-31 and 32-63 in one LDS cycle each over 32 banks
//     (MI355X_MICROARCH.md, LDS table), so the leading dimensions are chosen per half-wave:
//       C1 as [window row][query], ld 20:  write bank = 16 g + j (4 ld = 16 mod 32), read bank = 21 j - 16 g + const — both conflict-free;
//       C2 as [key][window row],   ld 37:  read bank = j + 16 g + 4 r + const (4 (ld - 1) = 16 mod 32) conflict-free; the write, bank
//       5 kk + 4 g + r, has one two-way conflict per half-wave (kk = 12 against kk = 0) — no ld serves both orientations.
//   * sc = (S^T + (C1 + C2)) / sqrt 3 in fp32: the shared softmax (attn_row_softmax) scales by log2(e) / 8, and 8 sqrt 3 = sqrt 192.
// Softmax, P rounding, O^T = V^T . P^T and the context store are attn16_block.h's, in its order.
//
// Short titles (S <= 32: two query blocks): a workgroup serves TWO (item, head) pairs at once, waves 0-1 one and waves 2-3 the other, each
// with its own LDS image (2 x 26 KiB + scratch); longer titles one pair per workgroup, query blocks round-robin over the four waves.
#include "attn16_block.h"

namespace {

constexpr float DISENT_SCALE = 0.57735026918962576f;     // 1 / sqrt 3: (.. / 8) of the shared softmax becomes (.. / sqrt 192)

template <int NT16>
struct DisentLds {
    typedef AttnLds<NT16> L;
    static constexpr int SP = L::SP;
    static constexpr int PAIRS = NT16 <= 2 ? 2 : 1;          // (item, head) pairs a workgroup serves at once
    static constexpr int TPP = 256 / PAIRS;                  // threads per pair
    static constexpr int WPP = 4 / PAIRS;                    // waves per pair
    static constexpr int MAXQB = (NT16 + WPP - 1) / WPP;     // 16-query blocks per wave
    static constexpr int RROWS = 2 * SP;                     // local table rows: w <-> d = w - SP + span
    static constexpr int PK_OFF = L::BYTES, PQ_OFF = PK_OFF + RROWS * 128, IMG = PQ_OFF + RROWS * 128;       // one pair's image
    static constexpr int C1_LD = 20, C2_LD = 37;
    static constexpr int C2_OFF = 32 * C1_LD * 4, SCR_WAVE = C2_OFF + 16 * C2_LD * 4;      // per wave: C1 [32][20] + C2 [16][37] fp32
    static constexpr int SCR_OFF = PAIRS * IMG, BYTES = SCR_OFF + 4 * SCR_WAVE;
    static_assert(L::BYTES % 16 == 0 && IMG % 16 == 0 && SCR_WAVE % 16 == 0, "16-byte aligned pieces");
    static_assert(BYTES <= 160 * 1024, "LDS of a CU");
};

// a wave's writes to its LDS scratch are visible to its own later reads (LDS serves one wave's operations in order); the fences keep the
// compiler from moving the accesses across, the wait drains the writes
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, int NT16>
__global__ __launch_bounds__(256) void attention16_disent_kernel(const typename T::elem* __restrict__ qkv, const typename T::elem* __restrict__ rel,
                                                                 const float* __restrict__ key_bias, typename T::elem* __restrict__ ctx,
                                                                 int64_t pairs, int S, int heads, int span) {
    typedef typename T::elem E;
    typedef typename T::v8 V8;
    typedef typename T::v4 V4;
    typedef DisentLds<NT16> DL;
    typedef typename DL::L L;
    constexpr int SP = L::SP, PAIRS = DL::PAIRS, TPP = DL::TPP, WPP = DL::WPP, RPP = TPP / 8;        // RPP: rows a pair's threads stage per pass
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = PAIRS == 2 ? wave >> 1 : 0, wv = wave - sub * WPP, ptid = tid - sub * TPP;
    // an odd number of pairs: the last workgroup's second half recomputes the last pair and stores nothing (every wave reaches the barrier)
    int64_t pair = (int64_t)blockIdx.x * PAIRS + sub;
    const bool live = pair < pairs;
    pair = live ? pair : pairs - 1;
    const int64_t item = pair / heads;
    const int h = (int)(pair - item * heads);
    const int D = heads * 64;
    const int j = lane & 15, g = lane >> 4;
    const int nqb = (S + 15) >> 4;
    const int c = ptid & 7, r0 = ptid >> 3;

    char* img = smem + sub * DL::IMG;
    char* sK = img;
    E* sVt = (E*)(img + L::VT_OFF);
    float* sKB = (float*)(img + L::KB_OFF);
    char* sPK = img + DL::PK_OFF;
    char* sPQ = img + DL::PQ_OFF;
    float* sC1 = (float*)(smem + DL::SCR_OFF + wave * DL::SCR_WAVE);
    float* sC2 = (float*)(smem + DL::SCR_OFF + wave * DL::SCR_WAVE + DL::C2_OFF);

    const E* qb_ = qkv + pair * 3 * S * 64;
    const E* kb_ = qb_ + (int64_t)S * 64;
    const E* vb_ = kb_ + (int64_t)S * 64;
    const E* pq_ = rel + (int64_t)h * 3 * 2 * span * 64;
    const E* pk_ = pq_ + (int64_t)2 * span * 64;

    // ---- stage the pair's image: key limits, K rows, V^T, the table rows.  Pad slots re-read the last real row (attn16.hip) ----
    for (int r = ptid; r < SP; r += TPP) sKB[r] = attn_key_limit(key_bias, (int)item, S, r);
#pragma unroll
    for (int r = r0; r < SP; r += RPP) {
        const V8 k = *(const V8*)(kb_ + (unsigned)((r < S ? r : S - 1) * 64 + c * 8));
        *(V8*)(sK + L::k_off(r, c)) = k;
    }
#pragma unroll
    for (int kg = r0; kg < SP / 4; kg += RPP) {
        V8 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = kg * 4 + r;
            v[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * 64 + c * 8));
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            V4 t;
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = v[r][e];
            *(V4*)L::vt_at(sVt, c * 8 + e, kg) = t;
        }
    }
    {
        const int dmax = 2 * span - 1;
#pragma unroll 4
        for (int w = r0; w < DL::RROWS; w += RPP) {
            int d = w - SP + span;
            d = d < 0 ? 0 : (d > dmax ? dmax : d);
            const V8 a = *(const V8*)(pk_ + (unsigned)(d * 64 + c * 8));
            const V8 b = *(const V8*)(pq_ + (unsigned)(d * 64 + c * 8));
            *(V8*)(sPK + L::k_off(w, c)) = a;
            *(V8*)(sPQ + L::k_off(w, c)) = b;
        }
    }
    __syncthreads();

#pragma unroll 1
    for (int i = 0; i < DL::MAXQB; ++i) {
        const int qb = wv + WPP * i;
        if (qb >= nqb) break;
        const int sq = qb * 16 + j;
        V8 qf[2];
        {
            const int sqc = sq < S ? sq : S - 1;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) qf[kk] = *(const V8*)(qb_ + (unsigned)(sqc * 64 + kk * 32 + g * 8));
        }
        f4 sc[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            V8 kf[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) kf[kk] = *(const V8*)(sK + L::k_off(t * 16 + j, kk * 4 + g));
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = T::mfma(kf[0], qf[0], acc);
            acc = T::mfma(kf[1], qf[1], acc);
            const int w0 = 16 * (qb - t) - 16 + SP;       // 0 .. 2 SP - 32: the window's 32 rows are inside the image
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int wr = w0 + 16 * u + j;
                V8 a[2], b[2];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    a[kk] = *(const V8*)(sPK + L::k_off(wr, kk * 4 + g));
                    b[kk] = *(const V8*)(sPQ + L::k_off(wr, kk * 4 + g));
                }
                f4 c1 = {0.f, 0.f, 0.f, 0.f}, c2 = {0.f, 0.f, 0.f, 0.f};
                c1 = T::mfma(a[0], qf[0], c1);
                c1 = T::mfma(a[1], qf[1], c1);
                c2 = T::mfma(b[0], kf[0], c2);
                c2 = T::mfma(b[1], kf[1], c2);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sC1[(16 * u + 4 * g + r) * DL::C1_LD + j] = c1[r];       // [window row][query]
                    sC2[j * DL::C2_LD + 16 * u + 4 * g + r] = c2[r];         // [key][window row]   (here j is the block's key)
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kk = 4 * g + r, wl = j - kk + 16;
                acc[r] = (acc[r] + (sC1[wl * DL::C1_LD + j] + sC2[kk * DL::C2_LD + wl])) * DISENT_SCALE;
            }
            wave_lds_sync();          // the next tile overwrites the scratch
            attn_apply_key_limit(acc, *(const f4*)(sKB + t * 16 + g * 4));
            sc[t] = acc;
        }
        const float inv = attn_row_softmax(sc, AttnKeepAll());

        f4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < NT16 / 2; ++kb) {
            const V8 pf = attn_round_p<T>(sc[2 * kb], sc[2 * kb + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = T::mfma(L::template vt_frag<V8>(sVt, dt, j, g, kb), pf, o[dt]);
        }
        attn_store_ctx<T>(ctx + (size_t)item * S * D, sq * D + h * 64, [&] { return g; }, o, inv, sq < S && live);
    }
}

// ---- CLS-query form: the last live block of the tower consumes the CLS row alone (attention_cls_kernel, attn16.hip) --------------------------
// For i = 0 both positional indices are d = span - j, so the row is Q0 . (K_j + PK[span - j]) + K_j . PQ[span - j].  One wave = one
// (item, head); phase 1 lanes over keys (8 lanes per key: 16 bytes of the K row and of the two table rows each, fp32 dot products), softmax
// statistics by wave shuffles, phase 2 lanes over (4 keys x 16 four-dim groups) streaming V rows.  P is rounded to the operand type before
// the PV product and the sum uses the unrounded values, as in the MFMA kernel.
template <typename T>
__global__ __launch_bounds__(256) void attention_cls_disent_kernel(const typename T::elem* __restrict__ qkv, const typename T::elem* __restrict__ rel,
                                                                   const float* __restrict__ key_bias, typename T::elem* __restrict__ ctx,
                                                                   int64_t pairs, int S, int heads, int span,
                                                                   const typename T::elem* __restrict__ q_cls) {
    typedef typename T::elem E;
    typedef typename T::v8 V8;
    typedef typename T::v4 V4;
    constexpr int SROW = 128;
    __shared__ float sP[4][SROW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
    if (pair >= pairs) return;
    const int64_t item = pair / heads;
    const int h = (int)(pair - item * heads);
    const E* qb_ = qkv + pair * 3 * S * 64;
    const E* kb_ = qb_ + (int64_t)S * 64;
    const E* vb_ = kb_ + (int64_t)S * 64;
    const E* pq_ = rel + (int64_t)h * 3 * 2 * span * 64;
    const E* pk_ = pq_ + (int64_t)2 * span * 64;
    const int kc = lane & 7, kr = lane >> 3;
    float q[8];
    {
        // q_cls: the CLS queries come from their own [items, heads*64] projection (the QKV GEMM wrote K and V only)
        const V8 t = q_cls ? *(const V8*)(q_cls + (item * heads + h) * 64 + kc * 8) : *(const V8*)(qb_ + kc * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = T::to_f32(t[e]);
    }
    float mx = -INFINITY;
    constexpr int KB = 4;                       // K rows (with their two table rows and mask values) per lane in flight
    for (int k0 = 0; k0 < S; k0 += 8 * KB) {
        V8 t[KB], pk[KB], pq[KB];
        float kbv[KB];
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            const int key = k0 + 8 * u + kr;
            const int kcl = key < S ? key : S - 1;
            t[u] = *(const V8*)(kb_ + (int64_t)kcl * 64 + kc * 8);
            pk[u] = *(const V8*)(pk_ + (int64_t)(span - kcl) * 64 + kc * 8);       // span - S + 1 .. span: inside the table (S <= span)
            pq[u] = *(const V8*)(pq_ + (int64_t)(span - kcl) * 64 + kc * 8);
            kbv[u] = key_bias ? key_bias[item * S + kcl] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            const int key = k0 + 8 * u + kr;
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float kv = T::to_f32(t[u][e]);
                a = fmaf(q[e], kv + T::to_f32(pk[u][e]), a);
                b = fmaf(kv, T::to_f32(pq[u][e]), b);
            }
            a += b;
            a += __shfl_xor(a, 1, 64);
            a += __shfl_xor(a, 2, 64);
            a += __shfl_xor(a, 4, 64);
            a *= DISENT_SCALE;
            if (key >= S) a = -INFINITY;
            else if (kbv[u] < 0.f) a = MASK_RAW;
            if (kc == 0 && key < SROW) sP[wave][key] = a;
            mx = fmaxf(mx, a);
        }
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0): the raw scores are in sP (each wave uses only its own row)
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < SROW / 64; ++i) {
        const int key = lane + 64 * i;
        const float a = key < S ? sP[wave][key] : -INFINITY;
        const float p = __builtin_amdgcn_exp2f((a - mx) * ATTN_C2);      // -inf -> 0 for the structural pad keys
        sum += p;
        sP[wave][key] = T::to_f32(T::from_f32(p));
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = 1.0f / sum;
    __builtin_amdgcn_s_waitcnt(0xc07f);           // lgkmcnt(0): this wave's sP writes (each wave reads only its own row)
    const int kg = lane >> 4, dq = lane & 15;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int VB = 8;
    for (int k0 = kg; k0 < S; k0 += 4 * VB) {
        V4 v[VB];
        float pr[VB];
#pragma unroll
        for (int u = 0; u < VB; ++u) {
            const int key = k0 + 4 * u;
            const int kcl = key < S ? key : S - 1;
            v[u] = *(const V4*)(vb_ + (int64_t)kcl * 64 + dq * 4);
            pr[u] = key < S ? sP[wave][kcl] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < VB; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(pr[u], T::to_f32(v[u][e]), acc[e]);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        acc[e] += __shfl_xor(acc[e], 16, 64);
        acc[e] += __shfl_xor(acc[e], 32, 64);
    }
    if (kg == 0) {
        V4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = T::from_f32(acc[e] * inv);
        *(V4*)(ctx + item * (int64_t)heads * 64 + h * 64 + dq * 4) = o;
    }
}

template <typename T, int NT16>
int launch_nt(const void* qkv, const void* rel, const float* key_bias, void* ctx, int64_t items, int S, int heads, int span, hipStream_t s) {
    typedef typename T::elem E;
    typedef DisentLds<NT16> DL;
    static OncePerDevice raised;
    if (raised.first())
        IISAN_HIP_OK(hipFuncSetAttribute((const void*)attention16_disent_kernel<T, NT16>, hipFuncAttributeMaxDynamicSharedMemorySize, DL::BYTES));
    const int64_t pairs = items * heads;
    dim3 grid((unsigned)ceil_div(pairs, DL::PAIRS)), block(256);
    hipLaunchKernelGGL((attention16_disent_kernel<T, NT16>), grid, block, DL::BYTES, s, (const E*)qkv, (const E*)rel, key_bias, (E*)ctx, pairs, S, heads, span);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

template <typename T>
int launch_t(const void* qkv, const void* rel, const float* key_bias, void* ctx, int64_t items, int S, int heads, int span, hipStream_t s) {
    if (S <= 32) return launch_nt<T, 2>(qkv, rel, key_bias, ctx, items, S, heads, span, s);
    if (S <= 64) return launch_nt<T, 4>(qkv, rel, key_bias, ctx, items, S, heads, span, s);
    return launch_nt<T, 8>(qkv, rel, key_bias, ctx, items, S, heads, span, s);
}

int check_disent(const char* what, const void* qkv, const void* rel, const void* ctx, int64_t items, int S, int heads, int span) {
    IISAN_CHECK_SHAPE(qkv && rel && ctx, "%s: null qkv, rel or ctx", what);
    IISAN_CHECK_SHAPE(items > 0 && heads > 0, "%s: empty problem", what);
    IISAN_CHECK_SHAPE(span >= 1 && span <= 256, "%s: span %d outside 1 .. 256", what, span);
    IISAN_CHECK_SHAPE(S >= 1 && S <= 128 && S <= span, "%s: sequence length %d outside 1 .. min(128, span = %d)", what, S, span);
    IISAN_CHECK_SHAPE(items * heads < (1ll << 31), "%s: grid too large", what);
    IISAN_CHECK_SHAPE((int64_t)S * heads * 64 < (1ll << 31), "%s: item of %d x %d elements too large", what, S, heads * 64);
    return IISAN_OK;
}

}  // namespace

int launch_attention16_disent(int dtype16, const void* qkv, const void* rel, const float* key_bias, void* ctx, int64_t items, int S, int heads,
                              int span, hipStream_t s) {
    IISAN_TRY(check_disent("attention16_disent", qkv, rel, ctx, items, S, heads, span));
    return dtype16 == IISAN_BF16 ? launch_t<BF16>(qkv, rel, key_bias, ctx, items, S, heads, span, s)
                                 : launch_t<F16>(qkv, rel, key_bias, ctx, items, S, heads, span, s);
}

int launch_attention_cls16_disent(int dtype16, const void* qkv, const void* rel, const float* key_bias, void* ctx_cls, int64_t items, int S,
                                  int heads, int span, hipStream_t s, const void* q_cls) {
    IISAN_TRY(check_disent("attention_cls16_disent", qkv, rel, ctx_cls, items, S, heads, span));
    const int64_t pairs = items * heads;
    dim3 grid((unsigned)ceil_div(pairs, 4)), block(256);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL((attention_cls_disent_kernel<BF16>), grid, block, 0, s, (const __bf16*)qkv, (const __bf16*)rel, key_bias, (__bf16*)ctx_cls,
                           pairs, S, heads, span, (const __bf16*)q_cls);
    else
        hipLaunchKernelGGL((attention_cls_disent_kernel<F16>), grid, block, 0, s, (const _Float16*)qkv, (const _Float16*)rel, key_bias,
                           (_Float16*)ctx_cls, pairs, S, heads, span, (const _Float16*)q_cls);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_attention16_disent(int32_t dtype16, const void* qkv, const void* rel, const float* key_bias, void* ctx, int64_t items,
                                        int32_t S, int32_t heads, int32_t span, void* stream) {
    return launch_attention16_disent(dtype16, qkv, rel, key_bias, ctx, items, S, heads, span, (hipStream_t)stream);
}

extern "C" int iisan_attention_cls16_disent(int32_t dtype16, const void* qkv, const void* rel, const float* key_bias, void* ctx_cls,
                                            int64_t items, int32_t S, int32_t heads, int32_t span, void* stream) {
    return launch_attention_cls16_disent(dtype16, qkv, rel, key_bias, ctx_cls, items, S, heads, span, (hipStream_t)stream, nullptr);
}
