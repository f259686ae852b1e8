// Train-mode dropout of the frozen BERT tower (opt-in: iisan_bert_forward_taps_dropout), as HF's BertModel applies it under
// model.train() (Code_Uncached/run.py:394): on the embedding output, on the attention probabilities (no renormalisation: the softmax
// denominator is that of the undropped row), and on the outputs of the two dense layers that add into the residual stream.
// Masks are counter-based (drop_scale, common.h): the keep factor of an element is a pure function of (seed, site, index) with
//   site 0 = embeddings, 1 + 3l = attention probabilities of block l, 2 + 3l = attention-output dense, 3 + 3l = FFN-output dense,
//   hidden sites:    index = (m T + t) 768 + c          attention sites: index = ((m H + h) T + q) T + k
// where m is the slot's position in the WHOLE call — so chunked and unchunked, indexed and direct calls, and the CLS-only last block
// and the all-token execution draw the same masks.  The eval-mode kernels (attn16.hip, rowops.hip) are not touched: every kernel here is
// a variant of its own, launched only when a dropout description with a non-zero probability is given.
#include "attn16_block.h"

// launches of this file's kernels: with the switch off a step leaves it at 0 — it runs the eval-mode launch sequence (tests, tools/bert_dropout_time.py)
static int64_t g_cnt_bert_drop = 0;
IISAN_DEV_COUNTER(bert_drop, g_cnt_bert_drop);

namespace {

// ---- attention with dropped probabilities -----------------------------------------------------------------------------------------
// ctx = (drop(P) V) with P = softmax(Q K^T / 8 + key_bias): the keep factor multiplies the exponentials that go into the P.V product,
// the row sum that normalises them is taken BEFORE it.  One workgroup = one (item, head): K (XOR-swizzled rows) and V^T (keys permuted
// inside groups of 32) of that head in LDS, one wave per 16-query block, scores of a whole row in registers (S <= 224: at most 14
// tiles) — the layouts, the MFMA mapping and the ORDER of every fp32 operation are those of attention16_kernel (attn16.hip): both are
// built from attn16_block.h, so that with the identity mask (p = 0) the result equals that kernel's bit for bit.  No register prefetch of the next head, one head per
// workgroup: the text tower's attention is a few per cent of its time (S = 30: two key tiles).
// CLS: only query 0 of every item (the last live block of the executor): q from `q_cls` [items, heads * 64] when given (the QKV
// product of that block wrote K and V only), ctx [items, heads * 64].  The mask is that of row q = 0 of the all-token form.
template <typename T, int NT16, bool CLS>
__global__ __launch_bounds__(256) void attention16_drop_kernel(const typename T::elem* __restrict__ qkv, const float* __restrict__ key_bias,
                                                               typename T::elem* __restrict__ ctx,
                                                               const typename T::elem* __restrict__ q_cls, int S, int heads,
                                                               DropCfg drop, int64_t slot0) {
    typedef typename T::elem E;
    typedef typename T::v8 V8;
    typedef typename T::v4 V4;
    typedef AttnLds<NT16> L;
    __shared__ __attribute__((aligned(16))) char smem[L::BYTES];
    char* sK = smem;
    E* sVt = (E*)(smem + L::VT_OFF);
    float* sKB = (float*)(smem + L::KB_OFF);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = blockIdx.x / heads, h = blockIdx.x - item * heads;
    const int D = heads * 64;
    const int j = lane & 15, g = lane >> 4;
    const int c = tid & 7, r0 = tid >> 3;
    const E* qb_ = qkv + ((int64_t)item * heads + h) * 3 * S * 64;
    const E* kb_ = qb_ + (int64_t)S * 64;
    const E* vb_ = kb_ + (int64_t)S * 64;

    // pad slots (row >= S) re-read the last real row: their scores are forced to -inf below, their P is exactly 0
#pragma unroll
    for (int p = 0; p < L::KP; ++p) {
        const int r = r0 + 32 * p;
        L::stage_k_row(sK, r, c, *(const V8*)(kb_ + (unsigned)((r < S ? r : S - 1) * 64 + c * 8)));
    }
#pragma unroll
    for (int p = 0; p < L::VP; ++p) {
        const int kg = r0 + 32 * p;
        if (kg < L::SP / 4) {
            V8 v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kg * 4 + r;
                v[r] = *(const V8*)(vb_ + (unsigned)((key < S ? key : S - 1) * 64 + c * 8));
            }
            L::template stage_v_group<T>(sVt, tid, p, v);
        }
    }
    for (int r = tid; r < L::SP; r += 256) sKB[r] = attn_key_limit(key_bias, item, S, r);
    __syncthreads();

    const int nqb = CLS ? 1 : (S + 15) >> 4;
    const uint64_t pair = (uint64_t)(slot0 + item) * (uint64_t)heads + (uint64_t)h;
#pragma unroll 1
    for (int qb = wave; qb < nqb; qb += 4) {
        const int sq = CLS ? 0 : qb * 16 + j;
        const int sqc = sq < S ? sq : S - 1;
        V8 qf[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (CLS) qf[kk] = q_cls ? *(const V8*)(q_cls + ((int64_t)item * heads + h) * 64 + kk * 32 + g * 8) : *(const V8*)(qb_ + kk * 32 + g * 8);
            else qf[kk] = *(const V8*)(qb_ + (unsigned)(sqc * 64 + kk * 32 + g * 8));
        }
        // S^T tiles: the lane holds query j, keys 16 t + 4 g + r (raw dot products; the 1/8 scale is folded into exp2)
        f4 sc[NT16];
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            V8 kf[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) kf[kk] = *(const V8*)(sK + L::k_off(t * 16 + j, kk * 4 + g));
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = T::mfma(kf[0], qf[0], acc);
            acc = T::mfma(kf[1], qf[1], acc);
            sc[t] = acc;
        }
#pragma unroll
        for (int t = 0; t < NT16; ++t) attn_apply_key_limit(sc[t], *(const f4*)(sKB + t * 16 + g * 4));
        // index of (query sq, key 0) at this site; pad queries (sq >= S) are never stored, pad keys have P = 0
        const uint64_t base = (pair * (uint64_t)S + (uint64_t)sq) * (uint64_t)S;
        const float inv = attn_row_softmax(sc, [&](int t, int r) {
            return drop_scale(drop.seed, drop.site, base + (uint64_t)(16 * t + 4 * g + r), drop.thr24, drop.inv_keep);
        });

        // O^T = V^T · drop(P)^T: the lane holds head dims 16 dt + 4 g + (0..3) of its query
        f4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = (f4){0.f, 0.f, 0.f, 0.f};
        constexpr int NPV = NT16 / 2;
#pragma unroll
        for (int kb = 0; kb < NPV; ++kb) {
            const V8 pf = attn_round_p<T>(sc[2 * kb], sc[2 * kb + 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = T::mfma(L::template vt_frag<V8>(sVt, dt, j, g, kb), pf, o[dt]);
        }
        if constexpr (NT16 % 2 == 1) {                 // keys SP-16 .. SP-1
            const V4 pt = attn_round_p_tail<T>(sc[NT16 - 1]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = Mfma16k16<T>::run(L::template vt_frag<V4>(sVt, dt, j, g, NT16 / 2), pt, o[dt]);
        }
        if (CLS) {
            if (j == 0) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    V4 ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = T::from_f32(o[dt][r] * inv);
                    *(V4*)(ctx + (int64_t)item * D + h * 64 + dt * 16 + g * 4) = ov;
                }
            }
        } else {
            attn_store_ctx<T>(ctx + (size_t)item * S * D, sq * D + h * 64, [&] { return g; }, o, inv, sq < S);
        }
    }
}

template <typename T, bool CLS>
int launch_attn_t(const void* qkv, const float* key_bias, void* ctx, const void* q_cls, int64_t items, int S, int heads,
                  const DropCfg& drop, int64_t slot0, hipStream_t s) {
    typedef typename T::elem E;
    dim3 grid((unsigned)(items * heads)), block(256);
#define IISAN_ATTN_DROP_CASE(NT) \
    hipLaunchKernelGGL((attention16_drop_kernel<T, NT, CLS>), grid, block, 0, s, (const E*)qkv, key_bias, (E*)ctx, (const E*)q_cls, S, heads, drop, slot0)
    if (S <= 32) IISAN_ATTN_DROP_CASE(2);
    else if (S <= 64) IISAN_ATTN_DROP_CASE(4);
    else if (S <= 128) IISAN_ATTN_DROP_CASE(8);
    else if (S <= 208) IISAN_ATTN_DROP_CASE(13);
    else IISAN_ATTN_DROP_CASE(14);
#undef IISAN_ATTN_DROP_CASE
    ++g_cnt_bert_drop;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

// ---- x = LN(x + drop(delta)) on the mixed residual stream ---------------------------------------------------------------------------
// The add + LayerNorm step behind the O / FC2 products (layernorm768_mixed_kernel with MX_D1 | MX_LN | MX_RESY [| MX_ALIAS], rowops.hip)
// with the keep factor applied to the 16-bit delta as it is read: no extra pass over HBM, no extra rounding of the delta.  CLS rows fp32
// in `xc` [items, 768], every other row fp16 in `x16`; ALIAS: out16 IS x16 (fp16 operands).  Half a wave per token row, a workgroup = 8
// consecutive tokens of one item.  row0 = index of the chunk's first token row in the whole call.
template <typename T, bool ALIAS>
__global__ __launch_bounds__(256) void add_ln_drop_mixed_kernel(_Float16* x16, float* xc, const typename T::elem* __restrict__ delta,
                                                                const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                                typename T::elem* out16, int64_t items, int Ttok, DropCfg drop,
                                                                int64_t row0) {
    typedef typename T::v8 V8;
    const int lane = threadIdx.x & 31, half = threadIdx.x >> 5;
    const int bpi = (Ttok + 7) >> 3;
    const int64_t item = blockIdx.x / bpi;
    const int tok = (int)(blockIdx.x - item * bpi) * 8 + half;
    if (tok >= Ttok) return;
    const int64_t row = item * Ttok + tok;
    const bool cls = tok == 0;                                            // uniform within the half-wave
    V8 d1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) d1[i] = __builtin_nontemporal_load((const V8*)(delta + row * 768 + i * 256 + lane * 8));
    float v[3][8];
    if (cls) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const f4 a = *(const f4*)(xc + item * 768 + i * 256 + lane * 8), c = *(const f4*)(xc + item * 768 + i * 256 + lane * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[i][e] = a[e]; v[i][4 + e] = c[e]; }
        }
    } else {
        h8 xh[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) xh[i] = __builtin_nontemporal_load((const h8*)(x16 + row * 768 + i * 256 + lane * 8));
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = (float)xh[i][e];
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint64_t idx = (uint64_t)(row0 + row) * 768u + (uint64_t)(i * 256 + lane * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] += drop_scale(drop.seed, drop.site, idx + e, drop.thr24, drop.inv_keep) * T::to_f32(d1[i][e]);
            s += v[i][e];
        }
    }
    auto sum32 = [](float t) {          // over the 32 lanes of the half-wave
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        return t;
    };
    const float mean = sum32(s) * (1.0f / 768.0f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(sum32(q) * (1.0f / 768.0f) + eps);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 8;
        const f4 g0 = *(const f4*)(g + c), g1 = *(const f4*)(g + c + 4), b0 = *(const f4*)(b + c), b1 = *(const f4*)(b + c + 4);
        float y[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = (v[i][e] - mean) * rstd * g0[e] + b0[e];
            y[4 + e] = (v[i][4 + e] - mean) * rstd * g1[e] + b1[e];
        }
        if (cls) {
            *(f4*)(xc + item * 768 + c) = (f4){y[0], y[1], y[2], y[3]};
            *(f4*)(xc + item * 768 + c + 4) = (f4){y[4], y[5], y[6], y[7]};
        } else if (!ALIAS) {
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)y[e];
            __builtin_nontemporal_store(o, (h8*)(x16 + row * 768 + c));
        }
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = T::from_f32(y[e]);
        *(V8*)(out16 + row * 768 + c) = o;
    }
}

// ---- the same on compact fp32 rows: the CLS rows of the last live block -------------------------------------------------------------
// x [rows, 768] fp32 in place, row r = the CLS token of item item0 + r: the mask index is that of TOKEN row (item0 + r) Ttok of the
// all-token execution.  out16 (optional): the 16-bit image of the result.  One wave per row (layernorm768_kernel, rowops.hip).
template <typename T>
__global__ __launch_bounds__(256) void add_ln_drop_rows_kernel(float* x, const typename T::elem* __restrict__ delta,
                                                               const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                               typename T::elem* __restrict__ out16, int64_t rows, DropCfg drop,
                                                               int64_t item0, int Ttok) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    f4 v[3];
    typename T::v4 d1[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = *(const f4*)(x + row * 768 + i * 256 + lane * 4);
        d1[i] = *(const typename T::v4*)(delta + row * 768 + i * 256 + lane * 4);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint64_t idx = (uint64_t)(item0 + row) * (uint64_t)Ttok * 768u + (uint64_t)(i * 256 + lane * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] += drop_scale(drop.seed, drop.site, idx + e, drop.thr24, drop.inv_keep) * T::to_f32(d1[i][e]);
        s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
    const float mean = wave_sum(s) * (1.0f / 768.0f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / 768.0f) + eps);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 4;
        const f4 gg = *(const f4*)(g + c), bb = *(const f4*)(b + c);
        f4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * gg[e] + bb[e];
        *(f4*)(x + row * 768 + c) = y;
        if (out16) {
            typename T::v4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = T::from_f32(y[e]);
            *(typename T::v4*)(out16 + row * 768 + c) = o;
        }
    }
}

// ---- embeddings: drop(LN(word[id] + pos[t] + type[0])) = hidden state 0 --------------------------------------------------------------
// bert_embed_ln_kernel (rowops.hip) for the mixed stream, with the keep factor applied to the fp32 LayerNorm output BEFORE it is rounded:
// every copy the executor keeps of the row — the 16-bit image H, the fp16 stream X16 (when it is not the image) and the fp32 CLS rows Xc
// that become tap 0 — holds the dropped value.  m0 = position of the chunk's first slot in the whole call.
template <typename T, bool IDX>
__global__ __launch_bounds__(256) void bert_embed_ln_drop_kernel(const int64_t* __restrict__ text, const float* __restrict__ word,
                                                                 const float* __restrict__ pos, const float* __restrict__ type0,
                                                                 const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                                 typename T::elem* __restrict__ H, float* __restrict__ key_bias,
                                                                 int64_t M, int W, int vocab, _Float16* __restrict__ X16,
                                                                 float* __restrict__ Xc, const int64_t* __restrict__ index, int64_t rows,
                                                                 DropCfg drop, int64_t m0) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M * W) return;
    const int64_t m = row / W;
    const int t = (int)(row % W);
    int64_t id, msk;
    if constexpr (IDX) {
        const int64_t sm = index[m];
        const bool pad = (uint64_t)sm >= (uint64_t)rows;      // a padding slot: never dereferenced, all-zero ids and mask
        id = pad ? 0 : text[sm * 2 * W + t];
        msk = pad ? 0 : text[sm * 2 * W + W + t];
    } else {
        id = text[m * 2 * W + t];
        msk = text[m * 2 * W + W + t];
    }
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    if (lane == 0) key_bias[row] = msk != 0 ? 0.0f : -1.0f;
    const float* wr = word + id * 768;
    const float* pr = pos + (int64_t)t * 768;
    f4 v[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 4;
        const f4 a = *(const f4*)(wr + c), p2 = *(const f4*)(pr + c), ty = *(const f4*)(type0 + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[i][e] = a[e] + p2[e] + ty[e];
        s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
    const float mean = wave_sum(s) * (1.0f / 768.0f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(wave_sum(q) * (1.0f / 768.0f) + eps);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 4;
        const f4 gg = *(const f4*)(g + c), bb = *(const f4*)(b + c);
        const uint64_t idx = (uint64_t)(m0 * W + row) * 768u + (uint64_t)c;
        f4 y;
        typename T::v4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = ((v[i][e] - mean) * rstd * gg[e] + bb[e]) * drop_scale(drop.seed, drop.site, idx + e, drop.thr24, drop.inv_keep);
            o[e] = T::from_f32(y[e]);
        }
        if (t == 0) {                        // CLS rows fp32 (compact), the others fp16
            *(f4*)(Xc + m * 768 + c) = y;
        } else if ((const void*)H != (const void*)X16) {     // (H == X16: the fp16 image is the stream — one store below covers every row)
            h4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = (_Float16)y[e];
            *(h4*)(X16 + row * 768 + c) = xh;
        }
        *(typename T::v4*)(H + row * 768 + c) = o;
    }
}

}  // namespace

int launch_attention16_drop(int dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int S, int heads,
                            const DropCfg& drop, int64_t slot0, bool cls_only, const void* q_cls, hipStream_t s) {
    IISAN_CHECK_SHAPE(items > 0 && S > 0 && heads > 0, "attention16_dropout: empty problem");
    IISAN_CHECK_SHAPE(S <= 224, "attention16_dropout: sequence length %d > 224 not supported", S);
    IISAN_CHECK_SHAPE(slot0 >= 0, "attention16_dropout: negative slot offset");
    IISAN_CHECK_SHAPE(items * heads < (1ll << 31), "attention16_dropout: grid too large");
    IISAN_CHECK_SHAPE((int64_t)S * heads * 64 < (1ll << 31), "attention16_dropout: item of %d x %d elements too large", S, heads * 64);
    if (dtype16 == IISAN_BF16)
        return cls_only ? launch_attn_t<BF16, true>(qkv, key_bias, ctx, q_cls, items, S, heads, drop, slot0, s)
                        : launch_attn_t<BF16, false>(qkv, key_bias, ctx, nullptr, items, S, heads, drop, slot0, s);
    return cls_only ? launch_attn_t<F16, true>(qkv, key_bias, ctx, q_cls, items, S, heads, drop, slot0, s)
                    : launch_attn_t<F16, false>(qkv, key_bias, ctx, nullptr, items, S, heads, drop, slot0, s);
}

int launch_add_ln_drop_mixed(int dtype16, bool alias, void* x16, float* xc, const void* delta16, const float* g, const float* b, float eps,
                             void* out16, int64_t items, int Ttok, const DropCfg& drop, int64_t row0, hipStream_t s) {
    if (items <= 0) return IISAN_OK;
    IISAN_CHECK_SHAPE(!alias || (dtype16 == IISAN_F16 && out16 == x16), "add_ln_drop_mixed: the aliased image needs fp16 operands and out16 == x16");
    const int64_t blocks = items * ((Ttok + 7) / 8);
    IISAN_CHECK_SHAPE(blocks < (1ll << 31), "add_ln_drop_mixed: grid too large");
    dim3 grid((unsigned)blocks), block(256);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL((add_ln_drop_mixed_kernel<BF16, false>), grid, block, 0, s, (_Float16*)x16, xc, (const __bf16*)delta16, g, b, eps, (__bf16*)out16, items, Ttok, drop, row0);
    else if (alias)
        hipLaunchKernelGGL((add_ln_drop_mixed_kernel<F16, true>), grid, block, 0, s, (_Float16*)x16, xc, (const _Float16*)delta16, g, b, eps, (_Float16*)out16, items, Ttok, drop, row0);
    else
        hipLaunchKernelGGL((add_ln_drop_mixed_kernel<F16, false>), grid, block, 0, s, (_Float16*)x16, xc, (const _Float16*)delta16, g, b, eps, (_Float16*)out16, items, Ttok, drop, row0);
    ++g_cnt_bert_drop;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_add_ln_drop_rows(int dtype16, float* x, const void* delta16, const float* g, const float* b, float eps, void* out16,
                            int64_t rows, const DropCfg& drop, int64_t item0, int Ttok, hipStream_t s) {
    if (rows <= 0) return IISAN_OK;
    dim3 grid((unsigned)ceil_div(rows, 4)), block(256);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL(add_ln_drop_rows_kernel<BF16>, grid, block, 0, s, x, (const __bf16*)delta16, g, b, eps, (__bf16*)out16, rows, drop, item0, Ttok);
    else
        hipLaunchKernelGGL(add_ln_drop_rows_kernel<F16>, grid, block, 0, s, x, (const _Float16*)delta16, g, b, eps, (_Float16*)out16, rows, drop, item0, Ttok);
    ++g_cnt_bert_drop;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_bert_embed_ln_drop(int dtype16, const int64_t* text, int64_t rows, const int64_t* index, const float* word, const float* pos,
                              const float* type0, const float* g, const float* b, float eps, void* H, float* key_bias, int64_t M, int W,
                              int vocab, void* X16, float* Xc, const DropCfg& drop, int64_t m0, hipStream_t s) {
    dim3 grid((unsigned)ceil_div(M * W, 4)), block(256);
#define IISAN_EMBED_DROP(T, E, IDX) \
    hipLaunchKernelGGL((bert_embed_ln_drop_kernel<T, IDX>), grid, block, 0, s, text, word, pos, type0, g, b, eps, (E*)H, key_bias, M, W, vocab, (_Float16*)X16, Xc, index, rows, drop, m0)
    if (dtype16 == IISAN_BF16) { if (index) IISAN_EMBED_DROP(BF16, __bf16, true); else IISAN_EMBED_DROP(BF16, __bf16, false); }
    else { if (index) IISAN_EMBED_DROP(F16, _Float16, true); else IISAN_EMBED_DROP(F16, _Float16, false); }
#undef IISAN_EMBED_DROP
    ++g_cnt_bert_drop;
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_attention16_dropout(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                                         int32_t heads, float p, uint64_t seed, int32_t site, int32_t cls_only, void* stream) {
    IISAN_CHECK_SHAPE(p >= 0.f && p < 1.f, "attention16_dropout: probability %.3f out of range", p);
    IISAN_CHECK_SHAPE(site >= 0, "attention16_dropout: negative site");
    return launch_attention16_drop(dtype16, qkv, key_bias, ctx, items, S, heads, make_drop(seed, (uint32_t)site, p), 0, cls_only != 0, nullptr,
                                   (hipStream_t)stream);
}
