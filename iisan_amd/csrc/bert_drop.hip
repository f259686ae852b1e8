// Train-mode dropout of the frozen BERT tower (opt-in: iisan_bert_forward_taps_dropout), as HF's BertModel applies it under
// model.train() (Code_Uncached/run.py:394): on the embedding output, on the attention probabilities (no renormalisation: the softmax
// denominator is that of the undropped row), and on the outputs of the two dense layers that add into the residual stream.
// Masks are counter-based (drop_scale, common.h): the keep factor of an element is a pure function of (seed, site, index) with
//   site 0 = embeddings, 1 + 3l = attention probabilities of block l, 2 + 3l = attention-output dense, 3 + 3l = FFN-output dense,
//   hidden sites:    index = (m T + t) 768 + c          attention sites: index = ((m H + h) T + q) T + k
// where m is the slot's position in the WHOLE call — so chunked and unchunked, indexed and direct calls, and the CLS-only last block
// and the all-token execution draw the same masks.
// This file holds the attention kernel, built from the per-block core it shares with the eval-mode kernels (attn16_block.h).  The three
// hidden sites are instantiations of the eval-mode row kernels with a keep functor (RowKeep, common.h; rowops.hip).  Either way a
// train-mode kernel is launched only when a dropout description with a non-zero probability is given, and the eval-mode instantiations
// compile to the code they had before the functor existed (profiles/rowops_shared_body.md).
#include "attn16_block.h"

// train-mode launches, this file's and those of rowops.hip: with the switch off a step leaves it at 0 — it runs the eval-mode launch
// sequence (tests, tools/bert_dropout_time.py)
static int64_t g_cnt_bert_drop = 0;
IISAN_DEV_COUNTER(bert_drop, g_cnt_bert_drop);
void iisan_count_bert_drop() { ++g_cnt_bert_drop; }

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

extern "C" int iisan_attention16_dropout(int32_t dtype16, const void* qkv, const float* key_bias, void* ctx, int64_t items, int32_t S,
                                         int32_t heads, float p, uint64_t seed, int32_t site, int32_t cls_only, void* stream) {
    IISAN_CHECK_SHAPE(p >= 0.f && p < 1.f, "attention16_dropout: probability %.3f out of range", p);
    IISAN_CHECK_SHAPE(site >= 0, "attention16_dropout: negative site");
    return launch_attention16_drop(dtype16, qkv, key_bias, ctx, items, S, heads, make_drop(seed, (uint32_t)site, p), 0, cls_only != 0, nullptr,
                                   (hipStream_t)stream);
}
