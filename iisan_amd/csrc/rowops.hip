// Row-wise HBM-bound kernels of the frozen encoders: LayerNorm, patch extraction, embedding gather, CLS taps.
// Roofline: HBM (one read + one write of each row); one wave64 per row, 16-byte lane accesses,
// wavefront-shuffle reductions, fp32 statistics (two-pass mean / centred variance in registers).
// The row width D is a template parameter of the LayerNorm / embedding kernels (D / 256 pieces per lane: 3 at 768 — ViT-B, BERT-base —
// 4 at 1024 — ViT-L, BERT-large — 5 at 1280 — ViT-H/14, the ViT executor only); their names keep the 768 they were written for.  Below 768 (128, 192, 256, 384: BERT-tiny, ViT-tiny,
// BERT-mini, ViT-small) a row takes fewer lanes, a compile-time quantity beside the piece count (row_lpr / row_np below), and several
// rows share a wave.  The kernels of the ViT's product route
// (fold_ln_weights, stream_stats_finalize, the MX_STAT / MX_BLK32 operand sets) are 768 wide only.
// Train-mode dropout of the BERT tower (opt-in, bert_drop.hip) runs the SAME three kernels — layernorm768_mixed_kernel,
// layernorm768_kernel, bert_embed_ln_kernel — with a keep functor as trailing template parameter and kernel argument (RowKeep,
// common.h): the keep factor multiplies the 16-bit delta as it is added, or the embedding's LayerNorm output before it is rounded.  The
// default RowKeepNone is empty and every use sits under `if constexpr (KEEP::on)`: the eval-mode instantiations compile to the
// instruction stream they had without it (tools/isa_compare.py --ignore-arg RowKeepNone; profiles/rowops_shared_body.md).  RowKeep is
// instantiated only where the BERT executor launches it, 768 wide (no other width has one): a launcher given a RowKeep for anything else refuses.
#include "common.h"

namespace {

// How a row of D elements lies over the lanes: D = LPR * NP * VEC — LPR lanes per row (a power of two), NP pieces of VEC elements (one
// 16-byte access of the narrowest operand) per lane.  `full` = the lanes a row gets from 768 on (a whole wave in the fp32 kernels, half a
// wave in the mixed one): D / (full * VEC) pieces there (3 at 768, 4 at 1024).  Below that a row gets fewer lanes and several rows share a
// wave — fp32 kernels: 128 = 32 x 1, 192 = 16 x 3, 256 = 64 x 1, 384 = 32 x 3; mixed kernel: 16 x 1, 8 x 3, 32 x 1, 16 x 3 — with NP in
// {1, 3}, every access still 16 bytes per lane and the xor reductions log2(LPR) steps.
constexpr int row_np(int D, int vec, int full) { return D % (full * vec) == 0 ? D / (full * vec) : ((D / vec) % 3 == 0 ? 3 : 1); }
constexpr int row_lpr(int D, int vec, int full) { return D / vec / row_np(D, vec, full); }
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
constexpr bool row_width_ok(int D, int vec, int full) {
    const int np = row_np(D, vec, full), lpr = row_lpr(D, vec, full);
    return lpr * np * vec == D && lpr >= 8 && lpr <= full && (lpr & (lpr - 1)) == 0 && np >= 1 && np <= 5;
}
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {          // over the LPR lanes of a row (LPR = 64: wave_sum)
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- (residual add +) LayerNorm over rows of D fp32 (HF nn.LayerNorm, eps inside the sqrt) ----------------------
// v = x + delta16 (delta optional: the 16-bit output of the preceding O / FC2 GEMM, so the fp32 read-modify-write of
// the residual stream happens HERE, in an HBM-bound kernel, instead of stalling the MFMA pipeline in a GEMM epilogue);
// sum32 <- v (optional, may alias x); out32 / out16 <- LN(v) (optional, out32 may alias x).  g == nullptr: add only.
// Which optional operands exist is COMPILE TIME (V bit 0: delta, 1: delta2, 2: sum32, 3: LayerNorm outputs): with run-time
// null tests every load sat behind its own branch and hipcc waited for each one before issuing the next — one load in flight
// per wave, six HBM round trips per row (ISA: load, s_waitcnt vmcnt(0), load, s_waitcnt vmcnt(0), ...).  Now all loads of a
// row are requested first.
// KEEP on (the CLS rows of BERT's last live block in train mode, V = 9): v = x + keep * delta, local row r = token row r0 + r * rs.
template <typename T, int V, int D = 768, typename KEEP = RowKeepNone>
__global__ __launch_bounds__(256) void layernorm768_kernel(const float* x, const typename T::elem* __restrict__ delta,
                                                           const typename T::elem* __restrict__ delta2,
                                                           const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                           float* sum32, typename T::elem* __restrict__ out16,
                                                           float* out32, int64_t rows, KEEP keep = KEEP()) {
    constexpr bool D1 = V & 1, D2 = (V & 2) != 0, SUM = (V & 4) != 0, LN = (V & 8) != 0;
    static_assert(!KEEP::on || (D1 && !D2 && !SUM && LN), "train mode: x = LN(x + keep * delta) alone (delta2 is never dropped)");
    constexpr int NP = row_np(D, 4, 64), LPR = row_lpr(D, 4, 64), PW = LPR * 4;        // 4-element pieces per lane: 3 (768) or 4 (1024) over a whole wave
    static_assert(row_width_ok(D, 4, 64), "row width: LPR * NP * 4 with LPR a power of two, at most 1024 (the row lives in registers)");
    static_assert(!KEEP::on || D == 768, "train mode: 768 wide only");
    const int lane = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);       // (every lane of a row leaves together)
    if (row >= rows) return;
    // The fp32 residual stream and the 16-bit deltas are read once and not touched again for gigabytes: non-temporal
    // accesses (measured: 220.7 -> 201.8 us average per launch over a step's 49 launches)
    const float* xr = x + row * D;
    f4 v[NP];
    typename T::v4 d1[NP], d2[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        v[i] = __builtin_nontemporal_load((const f4*)(xr + i * PW + lane * 4));
        if (D1) d1[i] = __builtin_nontemporal_load((const typename T::v4*)(delta + row * D + i * PW + lane * 4));
        if (D2) d2[i] = __builtin_nontemporal_load((const typename T::v4*)(delta2 + row * D + i * PW + lane * 4));
    }
    f4 gg[NP], bb[NP];
    if (LN) {
#pragma unroll
        for (int i = 0; i < NP; ++i) { gg[i] = *(const f4*)(g + i * PW + lane * 4); bb[i] = *(const f4*)(b + i * PW + lane * 4); }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if constexpr (KEEP::on) {
            const uint64_t idx = keep.index(row, D, i * PW + lane * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] += keep(idx + e) * T::to_f32(d1[i][e]);
        } else if (D1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] += T::to_f32(d1[i][e]);
        }
        if (D2) {       // added AFTER delta, in fp32: (x + delta) + delta2 — the same value as two passes produce
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] += T::to_f32(d2[i][e]);
        }
        if (SUM) __builtin_nontemporal_store(v[i], (f4*)(sum32 + row * D + i * PW + lane * 4));
        s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
    if (!LN) return;
    const float mean = row_sum<LPR>(s) * (1.0f / (float)D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(row_sum<LPR>(q) * (1.0f / (float)D) + eps);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = i * PW + lane * 4;
        f4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * gg[i][e] + bb[i][e];
        if (out32) *(f4*)(out32 + row * D + c) = y;
        if (out16) {
            typename T::v4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = T::from_f32(y[e]);
            *(typename T::v4*)(out16 + row * D + c) = o;
        }
    }
}


// ---- the same with a MIXED-PRECISION residual stream (round 4) ------------------------------------------------------
// The path consumes only the CLS row of every hidden state (Code_Uncached/model/model.py:210-213), and every token row already
// reaches the next GEMM through a 16-bit LayerNorm image.  So the residual stream is kept in fp32 for the CLS rows only
// (`xc` [items, D], compact: the taps are copies of it) and in fp16 for the patch / word rows (`x16` [rows, D]; always
// IEEE half, whatever the MFMA operand type — bf16 would keep 8 bits).  A non-CLS row's rounding (2^-11, once per block)
// reaches the CLS row only through the attention average over the item's tokens: measured on the golden ViT-B inputs with
// fp32 arithmetic everywhere else, +9e-5 relative on every tap (all rows in fp16: 6.8e-4) against the 8.8e-4 the 16-bit operands
// cost and the 1.5e-3 budget.  Bytes per token row and ViT block: LN1 10 + LN2 6 = 16 instead of 14 + 8 = 22 (BERT: 8
// instead of 12 per LayerNorm) in kernels that run at the HBM rate.
// HALF a wave per token row (32 lanes x D / 256 = three or four 8-element pieces), a workgroup = 8 consecutive tokens of ONE item (the CLS test costs no
// division per lane): every access of the fp16 stream, the 16-bit deltas and the 16-bit image is a full 16-byte lane access.  (The
// first version gave a row to a whole wave — 12 elements per lane as three 8-byte pieces: 4.3 TB/s on LN1 where the fp32 kernel's
// 16-byte accesses reach 6.7; MI355X_MICROARCH.md: 8-byte accesses run at 0.54-0.70 x the 16-byte rate.)  V: which operands exist.
// KEEP on (BERT's x = LN(x + d) in train mode): the keep factor multiplies the 16-bit delta as it is added — no extra pass over HBM, no
// extra rounding of the delta; the CLS rows take it like every other row.
template <typename T, int V, int D = 768, typename KEEP = RowKeepNone>
__global__ __launch_bounds__(256) void layernorm768_mixed_kernel(const float* __restrict__ x32, _Float16* x16, float* xc,
                                                                 const typename T::elem* __restrict__ delta,
                                                                 const typename T::elem* __restrict__ delta2,
                                                                 const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                                 typename T::elem* __restrict__ out16, int64_t items, int Ttok,
                                                                 float* __restrict__ stat, KEEP keep = KEEP()) {
    constexpr bool D1 = (V & MX_D1) != 0, D2 = (V & MX_D2) != 0, LN = (V & MX_LN) != 0, RESV = (V & MX_RESV) != 0,
                   RESY = (V & MX_RESY) != 0, SRC32 = (V & MX_SRC32) != 0, CLSONLY = (V & MX_CLSONLY) != 0, POSROW = (V & MX_POSROW) != 0,
                   STAT = (V & MX_STAT) != 0, ALIAS = (V & MX_ALIAS) != 0, BLK32 = (V & MX_BLK32) != 0;
    static_assert(!BLK32 || (STAT && SRC32), "block-major stream: written by the ViT's first add only (the products do the rest)");
    // 8-element pieces per lane: 3 (768) or 4 (1024) over half a wave.  TPW tokens per workgroup: 8 from 768 on, 8 * 32 / LPR below
    constexpr int NP = row_np(D, 8, 32), LPR = row_lpr(D, 8, 32), PW = LPR * 8, TPW = 256 / LPR, TSH = ilog2(TPW);
    static_assert(row_width_ok(D, 8, 32), "row width: LPR * NP * 8 with LPR a power of two, at most 1024 (the row lives in registers)");
    static_assert(D == 768 || !(STAT || BLK32), "the product route's stream (row statistics, block-major rows) is 768 wide");
    static_assert(!KEEP::on || D == 768, "train mode: 768 wide only");
    static_assert(!KEEP::on || (V & ~MX_ALIAS) == (MX_D1 | MX_LN | MX_RESY), "train mode: x = LN(x + keep * delta) alone (delta2 is never dropped)");
    typedef typename T::v8 V8;
    const int lane = threadIdx.x & (LPR - 1), half = threadIdx.x / LPR;  // TPW rows per workgroup (8 half-waves from 768 on)
    int64_t item;
    int tok;
    if (CLSONLY) {
        item = (int64_t)blockIdx.x * TPW + half; tok = 0;
        if (item >= items) return;
    } else {
        // a workgroup = TPW consecutive tokens of ONE item (bpi workgroups per item, the last one ragged: tok >= Ttok leaves): no row of
        // it crosses the item boundary, and the CLS row is the one with tok == 0 — no division per lane
        const int bpi = (Ttok + TPW - 1) >> TSH;
        item = blockIdx.x / bpi;
        tok = (int)(blockIdx.x - item * bpi) * TPW + half;
        if (tok >= Ttok) return;
    }
    const int64_t row = item * Ttok + tok;
    const bool cls = tok == 0;                                            // uniform within the LPR lanes of a row
    V8 d1[NP], d2[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if (D1) d1[i] = __builtin_nontemporal_load((const V8*)(delta + row * D + i * PW + lane * 8));
        if (D2) d2[i] = __builtin_nontemporal_load((const V8*)(delta2 + row * D + i * PW + lane * 8));
    }
    float v[NP][8];
    if (cls) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const f4 a = *(const f4*)(xc + item * D + i * PW + lane * 8), c = *(const f4*)(xc + item * D + i * PW + lane * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[i][e] = a[e]; v[i][4 + e] = c[e]; }
        }
    } else if (SRC32) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int64_t srow = POSROW ? (int64_t)tok : row;            // POSROW: the position-embedding table (L2-resident), by token
            const f4 a = POSROW ? *(const f4*)(x32 + srow * D + i * PW + lane * 8) : __builtin_nontemporal_load((const f4*)(x32 + srow * D + i * PW + lane * 8));
            const f4 c = POSROW ? *(const f4*)(x32 + srow * D + i * PW + lane * 8 + 4) : __builtin_nontemporal_load((const f4*)(x32 + srow * D + i * PW + lane * 8 + 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[i][e] = a[e]; v[i][4 + e] = c[e]; }
        }
    } else {
        h8 xh[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) xh[i] = __builtin_nontemporal_load((const h8*)(x16 + row * D + i * PW + lane * 8));
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = (float)xh[i][e];
    }
    // STAT: the fp16 stream is the next product's A operand — the CLS rows go there too, and the statistics are those of the
    // ROUNDED row (what the product multiplies); val is rounded in place
    auto put_resid = [&](int i, float (&val)[8]) {
        if (cls) {
            *(f4*)(xc + item * D + i * PW + lane * 8) = (f4){val[0], val[1], val[2], val[3]};
            *(f4*)(xc + item * D + i * PW + lane * 8 + 4) = (f4){val[4], val[5], val[6], val[7]};
        }
        if ((!cls || STAT) && !ALIAS) {
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)val[e];
            // read again by the GEMM that follows (MX_BLK32: block-major, common.h — the lane's 8 columns are one 16-byte granule of it)
            if (STAT) *(h8*)(x16 + (BLK32 ? blk32_byte(row, i * PW + lane * 8, D) >> 1 : row * D + i * PW + lane * 8)) = o;
            else __builtin_nontemporal_store(o, (h8*)(x16 + row * D + i * PW + lane * 8));
            if (STAT) {
#pragma unroll
                for (int e = 0; e < 8; ++e) val[e] = (float)o[e];
            }
        }
    };
    float s = 0.f;
    const bool use_d = !(POSROW && cls);          // POSROW: the CLS slot of the patch-embedding buffer was never written
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        if constexpr (KEEP::on) {
            const uint64_t idx = keep.index(row, D, i * PW + lane * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] += keep(idx + e) * T::to_f32(d1[i][e]);
        } else if (D1 && use_d) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] += T::to_f32(d1[i][e]);
        }
        if (D2 && use_d) {       // added AFTER delta, in fp32: (x + delta) + delta2
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] += T::to_f32(d2[i][e]);
        }
        if (RESV && (STAT || !(POSROW && cls))) put_resid(i, v[i]);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += v[i][e];
    }
    if (!LN && !STAT) return;
    auto sum32 = [](float t) {          // over the LPR lanes of the row (32: the half-wave)
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        return t;
    };
    const float mean = sum32(s) * (1.0f / (float)D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(sum32(q) * (1.0f / (float)D) + eps);
    if (STAT) {
        if (lane == 0) stat[row] = rstd;
        return;
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = i * PW + lane * 8;
        const f4 g0 = *(const f4*)(g + c), g1 = *(const f4*)(g + c + 4), b0 = *(const f4*)(b + c), b1 = *(const f4*)(b + c + 4);
        float y[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = (v[i][e] - mean) * rstd * g0[e] + b0[e];
            y[4 + e] = (v[i][4 + e] - mean) * rstd * g1[e] + b1[e];
        }
        if (RESY) put_resid(i, y);
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = T::from_f32(y[e]);
        *(V8*)(out16 + row * D + c) = o;
    }
}

// ---- the opening step of a CLIP vision tower: embeddings -> pre-LayerNorm -> stream, and block 0's LN1 image, in one pass -------------
// x0 = LN_pre(v),  v = pos[tok] + patch embedding (16-bit, `patch16`: the EPI_PATCH16 product) — or, on a CLS row, cls + pos[0], which
// vit_cls_rows_kernel has left in xc.  x0 is hidden state 0 (`hidden_states[0]` of HF's CLIPVisionTransformer is the output of
// pre_layrnorm) and becomes the mixed residual stream exactly as layernorm768_mixed_kernel writes it: fp32 in xc for the CLS rows (tap 0
// is a copy of it), fp16 in x16 for the others.  The same lanes then normalise x0 — the fp32 values in their registers, not the rounded
// stream, as every LN1 of the image route does — with block 0's ln1 and write the 16-bit image `out16`.  Row layout, workgroup shape and
// reductions are those of the mixed kernel (half a wave per row from 768 on); four reductions per row instead of two, one read of the
// row, no second launch.
template <typename T, int D>
__global__ __launch_bounds__(256) void clip_open_kernel(const float* __restrict__ pos, _Float16* __restrict__ x16, float* xc,
                                                        const typename T::elem* __restrict__ patch16,
                                                        const float* __restrict__ pg, const float* __restrict__ pb,
                                                        const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                        typename T::elem* __restrict__ out16, int64_t items, int Ttok) {
    constexpr int NP = row_np(D, 8, 32), LPR = row_lpr(D, 8, 32), PW = LPR * 8, TPW = 256 / LPR, TSH = ilog2(TPW);
    static_assert(row_width_ok(D, 8, 32), "row width: LPR * NP * 8 with LPR a power of two, at most 1280 (the row lives in registers)");
    typedef typename T::v8 V8;
    const int lane = threadIdx.x & (LPR - 1), half = threadIdx.x / LPR;
    const int bpi = (Ttok + TPW - 1) >> TSH;          // a workgroup = TPW consecutive tokens of ONE item, as in the mixed kernel
    const int64_t item = blockIdx.x / bpi;
    const int tok = (int)(blockIdx.x - item * bpi) * TPW + half;
    if (item >= items || tok >= Ttok) return;
    const int64_t row = item * Ttok + tok;
    const bool cls = tok == 0;                        // uniform within the LPR lanes of a row
    float v[NP][8];
    if (cls) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const f4 a = *(const f4*)(xc + item * D + i * PW + lane * 8), c = *(const f4*)(xc + item * D + i * PW + lane * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[i][e] = a[e]; v[i][4 + e] = c[e]; }
        }
    } else {
        V8 d1[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) d1[i] = __builtin_nontemporal_load((const V8*)(patch16 + row * D + i * PW + lane * 8));
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const f4 a = *(const f4*)(pos + (int64_t)tok * D + i * PW + lane * 8), c = *(const f4*)(pos + (int64_t)tok * D + i * PW + lane * 8 + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[i][e] = a[e] + T::to_f32(d1[i][e]); v[i][4 + e] = c[e] + T::to_f32(d1[i][4 + e]); }
        }
    }
    auto sum = [](float t) {            // over the LPR lanes of the row
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        return t;
    };
    // v <- LayerNorm(v; gamma, beta) in place: two-pass mean / centred variance in registers, like every row kernel here
    auto normalise = [&](const float* __restrict__ gamma, const float* __restrict__ beta) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[i][e];
        const float mean = sum(s) * (1.0f / (float)D);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NP; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = v[i][e] - mean;
                q += d * d;
            }
        const float rstd = rsqrtf(sum(q) * (1.0f / (float)D) + eps);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int c = i * PW + lane * 8;
            const f4 g0 = *(const f4*)(gamma + c), g1 = *(const f4*)(gamma + c + 4), b0 = *(const f4*)(beta + c), b1 = *(const f4*)(beta + c + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[i][e] = (v[i][e] - mean) * rstd * g0[e] + b0[e];
                v[i][4 + e] = (v[i][4 + e] - mean) * rstd * g1[e] + b1[e];
            }
        }
    };
    normalise(pg, pb);                  // x0
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = i * PW + lane * 8;
        if (cls) {
            *(f4*)(xc + item * D + c) = (f4){v[i][0], v[i][1], v[i][2], v[i][3]};
            *(f4*)(xc + item * D + c + 4) = (f4){v[i][4], v[i][5], v[i][6], v[i][7]};
        } else {
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)v[i][e];
            __builtin_nontemporal_store(o, (h8*)(x16 + row * D + c));
        }
    }
    normalise(g, b);                    // LN1(x0) of block 0
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        V8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = T::from_f32(v[i][e]);
        *(V8*)(out16 + row * D + i * PW + lane * 8) = o;
    }
}

// per-channel normalisation of the uint8 sources of the patch extraction below: none (the reference's (.5, .5) transform, the code as it
// was) or (p / 255 - mean[c]) / std[c] for 3 channels (a pretrained CLIP's own statistics; iisan_vit_weights::norm_mean / norm_std)
struct PixNormNone { static constexpr bool on = false; };
struct PixNorm {
    static constexpr bool on = true;
    float mean[3], std[3];
    __device__ __forceinline__ float operator()(float u, int c) const {
        const float mu = c == 0 ? mean[0] : c == 1 ? mean[1] : mean[2], sd = c == 0 ? std[0] : c == 1 ? std[1] : std[2];
        return __fdiv_rn(__fdiv_rn(u, 255.0f) - mu, sd);
    }
};

// ---- ViT patch extraction: images fp32 [M,C,R,R] -> patch matrix 16-bit [M*P, C*p*p], col = c*p*p + iy*p + ix ----
// one thread = 8 consecutive ix (two float4 reads, one 16-byte store)
// SRC = float: already normalised pixels; SRC = uint8_t: raw pixels, normalised here exactly as the reference's
// transform does in fp32 — ToTensor (x/255) then Normalize(mean .5, std .5) (`Code_Uncached/data_utils/dataset.py:46-50`)
// — so the 16-bit patch matrix is bit-identical to the fp32 route while the image crosses PCIe/HBM at a quarter the size.
// IDX (uint8 only): `img` is a resident catalogue [rows, C, R, R] and item m reads row index[m]; any value outside [0, rows) is a
// padding slot — never dereferenced, its fragment is the all-zero NORMALISED image the reference ships for pad slots
// (`Code_Uncached/data_utils/dataset.py:73`; no uint8 pixel normalises to 0).  The plain instantiations compile as before.
// NRM (uint8 only; PixNorm above): per-channel statistics in place of (.5, .5).  The default PixNormNone is empty and its one use sits
// under `if constexpr (NRM::on)`, like the keep functor of the row kernels.
template <typename T, typename SRC, bool IDX = false, typename NRM = PixNormNone>
__global__ __launch_bounds__(256) void vit_im2col_kernel(const SRC* __restrict__ img, typename T::elem* __restrict__ out,
                                                         int64_t M, int C, int R, int p,
                                                         const int64_t* __restrict__ index = nullptr, int64_t rows = 0, NRM nrm = NRM()) {
    const int per_row = C * p * p / 8;        // threads per patch row
    const int gp = R / p;                      // patches per image side
    const int64_t total = M * gp * gp * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % per_row);
        const int64_t pr = i / per_row;        // patch row index = m*P + py*gp + px
        const int col = t * 8;
        const int c = col / (p * p), rem = col % (p * p), iy = rem / p, ix = rem % p;
        const int64_t m = pr / (gp * gp);
        const int pp = (int)(pr % (gp * gp)), py = pp / gp, px = pp % gp;
        int64_t sm = m;
        bool pad = false;
        if constexpr (IDX) {
            sm = index[m];
            pad = (uint64_t)sm >= (uint64_t)rows;       // negative or >= rows
            if (pad) sm = 0;                            // keeps the address arithmetic below in range; never loaded
        }
        const SRC* src = img + ((sm * C + c) * R + (py * p + iy)) * (int64_t)R + px * p + ix;
        f4 a, b2;
        if (IDX && pad) {
            a = f4{0.f, 0.f, 0.f, 0.f};
            b2 = a;
        } else if constexpr (sizeof(SRC) == 4) {
            a = *(const f4*)src;
            b2 = *(const f4*)(src + 4);
        } else {
            typedef uint8_t U8 __attribute__((ext_vector_type(8)));
            const U8 u = *(const U8*)src;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if constexpr (NRM::on) {
                    a[e] = nrm((float)u[e], c);
                    b2[e] = nrm((float)u[4 + e], c);
                } else {
                    a[e] = __fdiv_rn(__fdiv_rn((float)u[e], 255.0f) - 0.5f, 0.5f);
                    b2[e] = __fdiv_rn(__fdiv_rn((float)u[4 + e], 255.0f) - 0.5f, 0.5f);
                }
            }
        }
        typename T::v8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = T::from_f32(a[e]);
            o[4 + e] = T::from_f32(b2[e]);
        }
        *(typename T::v8*)(out + pr * (int64_t)(C * p * p) + col) = o;
    }
}

// The same for a patch side that is no multiple of 8 (ViT-H/14: p = 14, C p p = 588): the patch row is ZERO-PADDED to `ldp` columns, the next
// multiple of 64 (640), as the packed patch weight is, so the patch-embedding product keeps K % 64 == 0.  One thread = 8 consecutive
// columns of the padded row (one 16-byte store), each read on its own: a run of 8 columns crosses pixel rows of 14.  The arithmetic per pixel
// — the two __fdiv_rn of the uint8 source, the zero fragment of an indexed pad slot — is that of the kernel above.
template <typename T, typename SRC, bool IDX = false, typename NRM = PixNormNone>
__global__ __launch_bounds__(256) void vit_im2col_pad_kernel(const SRC* __restrict__ img, typename T::elem* __restrict__ out,
                                                             int64_t M, int C, int R, int p, int ldp,
                                                             const int64_t* __restrict__ index = nullptr, int64_t rows = 0, NRM nrm = NRM()) {
    const int pd = C * p * p, per_row = ldp / 8;
    const int gp = R / p;
    const int64_t total = M * gp * gp * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i % per_row);
        const int64_t pr = i / per_row;        // patch row index = m*P + py*gp + px
        const int64_t m = pr / (gp * gp);
        const int pp = (int)(pr % (gp * gp)), py = pp / gp, px = pp % gp;
        int64_t sm = m;
        bool pad = false;
        if constexpr (IDX) {
            sm = index[m];
            pad = (uint64_t)sm >= (uint64_t)rows;       // negative or >= rows: never loaded
            if (pad) sm = 0;
        }
        typename T::v8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int col = t * 8 + e;
            float a = 0.f;
            if (col < pd && !(IDX && pad)) {            // columns pd .. ldp - 1: the zero padding
                const int c = col / (p * p), rem = col % (p * p), iy = rem / p, ix = rem % p;
                const SRC v = img[((sm * C + c) * R + (py * p + iy)) * (int64_t)R + px * p + ix];
                if constexpr (sizeof(SRC) == 4) a = v;
                else if constexpr (NRM::on) a = nrm((float)v, c);
                else a = __fdiv_rn(__fdiv_rn((float)v, 255.0f) - 0.5f, 0.5f);
            }
            o[e] = T::from_f32(a);
        }
        *(typename T::v8*)(out + pr * (int64_t)ldp + t * 8) = o;
    }
}

// CLS rows of the token matrix: X[m*T] = cls + pos[0]
__global__ void vit_cls_rows_kernel(float* __restrict__ X, const float* __restrict__ cls, const float* __restrict__ pos,
                                    int64_t M, int T, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * D) return;
    const int64_t m = i / D;
    const int d = (int)(i % D);
    X[m * T * D + d] = cls[d] + pos[d];
}

// ---- BERT embeddings: LN(word[id] + pos[t] + type[0]) -> X fp32 + H 16-bit; key bias from the attention mask ------
// IDX: `text` is a resident table [rows, 2W] and item m reads row index[m]; a value outside [0, rows) is a padding slot — never
// dereferenced, all-zero ids and mask (what `dataset.py:79-84` ships for pad slots).
// KEEP on (train mode): drop(LN(...)) — the keep factor multiplies the fp32 LayerNorm output BEFORE it is rounded, so every copy the
// executor keeps of the row (the 16-bit image H, the fp16 stream X16, the fp32 CLS rows Xc that become tap 0) holds the dropped value.
// DEB (DeBERTa-v2/v3, HF DebertaV2Embeddings with position_biased_input = False and type_vocab_size = 0): LN(word[id]) * mask — no position and
// no type table (pos / type0 are not read), and the row of a masked token is exactly zero.  The key bias is written as for BERT.  The
// instantiation rides on the KEEP parameter (RowKeepDeberta: no dropout, eval mode only): the kernel's template list, and with it the
// symbol names of the BERT instantiations, stay as they are.
struct RowKeepDeberta { static constexpr bool on = false; };
template <class K> struct EmbedIsDeberta { static constexpr bool value = false; };
template <> struct EmbedIsDeberta<RowKeepDeberta> { static constexpr bool value = true; };
template <typename T, bool IDX = false, int D = 768, typename KEEP = RowKeepNone>
__global__ __launch_bounds__(256) void bert_embed_ln_kernel(const int64_t* __restrict__ text, const float* __restrict__ word,
                                                            const float* __restrict__ pos, const float* __restrict__ type0,
                                                            const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                            float* __restrict__ X, typename T::elem* __restrict__ H,
                                                            float* __restrict__ key_bias, int64_t M, int W, int vocab,
                                                            _Float16* __restrict__ X16, float* __restrict__ Xc,
                                                            const int64_t* __restrict__ index = nullptr, int64_t rows = 0,
                                                            KEEP keep = KEEP()) {
    constexpr int NP = row_np(D, 4, 64), LPR = row_lpr(D, 4, 64), PW = LPR * 4;        // as layernorm768_kernel
    static_assert(row_width_ok(D, 4, 64), "row width: LPR * NP * 4 with LPR a power of two, at most 1024");
    static_assert(!KEEP::on || D == 768, "train mode: 768 wide only");
    constexpr bool DEB = EmbedIsDeberta<KEEP>::value;
    const int lane = threadIdx.x & (LPR - 1);
    const int64_t row = (int64_t)blockIdx.x * (256 / LPR) + (threadIdx.x / LPR);
    if (row >= M * W) return;
    const int64_t m = row / W;
    const int t = (int)(row % W);
    int64_t id, msk;
    if constexpr (IDX) {
        const int64_t sm = index[m];
        const bool pad = (uint64_t)sm >= (uint64_t)rows;
        id = pad ? 0 : text[sm * 2 * W + t];
        msk = pad ? 0 : text[sm * 2 * W + W + t];
    } else {
        id = text[m * 2 * W + t];
        msk = text[m * 2 * W + W + t];
    }
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    if (lane == 0) key_bias[row] = msk != 0 ? 0.0f : -1.0f;
    const float* wr = word + id * D;
    const float* pr = DEB ? nullptr : pos + (int64_t)t * D;
    f4 v[NP];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = i * PW + lane * 4;
        if constexpr (DEB) {
            v[i] = *(const f4*)(wr + c);
        } else {
            const f4 a = *(const f4*)(wr + c), p2 = *(const f4*)(pr + c), ty = *(const f4*)(type0 + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = a[e] + p2[e] + ty[e];
        }
        s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
    }
    const float mean = row_sum<LPR>(s) * (1.0f / (float)D);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = v[i][e] - mean;
            q += d * d;
        }
    const float rstd = rsqrtf(row_sum<LPR>(q) * (1.0f / (float)D) + eps);
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = i * PW + lane * 4;
        const f4 gg = *(const f4*)(g + c), bb = *(const f4*)(b + c);
        f4 y;
        typename T::v4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            y[e] = (v[i][e] - mean) * rstd * gg[e] + bb[e];
            if constexpr (KEEP::on) y[e] *= keep(keep.index(row, D, c) + e);
            if constexpr (DEB) y[e] = msk != 0 ? y[e] : 0.f;
            o[e] = T::from_f32(y[e]);
        }
        if (X) {
            *(f4*)(X + row * D + c) = y;
        } else if (t == 0) {                 // mixed-precision residual stream: CLS rows fp32 (compact), the others fp16
            *(f4*)(Xc + m * D + c) = y;
        } else if ((const void*)H != (const void*)X16) {     // (H == X16: the fp16 image is the stream — one store below covers every row)
            typedef _Float16 hv4 __attribute__((ext_vector_type(4)));
            hv4 xh;
#pragma unroll
            for (int e = 0; e < 4; ++e) xh[e] = (_Float16)y[e];
            *(hv4*)(X16 + row * D + c) = xh;
        }
        *(typename T::v4*)(H + row * D + c) = o;
    }
}

// taps[m, k, :] = X[m*T, :]   (CLS row of every item; Code_Uncached/model/model.py:212-213)
__global__ void gather_cls_kernel(const float* __restrict__ X, float* __restrict__ taps, int64_t M, int T, int D,
                                  int n_taps, int k) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // float4 index
    const int d4 = D / 4;
    if (i >= M * d4) return;
    const int64_t m = i / d4;
    const int c = (int)(i % d4) * 4;
    *(f4*)(taps + (m * n_taps + k) * D + c) = *(const f4*)(X + m * T * D + c);
}

// 16-bit rows: out[m, :] = H[m*T, :]  (CLS rows of a token-major 16-bit activation), 16 bytes per thread
__global__ void gather_rows16_kernel(const uint4* __restrict__ H, uint4* __restrict__ out, int64_t M, int T, int D8) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * D8) return;
    const int64_t m = i / D8;
    const int c = (int)(i - m * D8);
    out[m * D8 + c] = H[m * T * D8 + c];
}

template <typename T>
__global__ void cast16_kernel(const float* __restrict__ src, typename T::elem* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = T::from_f32(src[i]);
}

}  // namespace

// The instantiated row widths: 768 / 1024 (ViT-B / BERT-base, ViT-L / BERT-large) and the narrow towers' 128, 192, 256, 384 (BERT-tiny, ViT-tiny,
// BERT-mini, ViT-small).  The refusal names the width it was given and 768 and 1024 first.
// 1280 (ViT-H/14: five pieces per lane) is instantiated like the others; the executors take it on the ViT alone (encoders.hip, check_common).
bool row_width_instantiated(int w) { return w == 768 || w == 1024 || w == 128 || w == 192 || w == 256 || w == 384 || w == 1280; }
#define ROW_WIDTH_MSG "row width %d not instantiated (768 and 1024 are, and 128, 192, 256, 384, 1280)"
// one switch over the widths: X(W, A) is the launch at the compile-time width W (A: whatever else the launch is a template of).
// ROW_WIDTH_SWITCH_64: the widths of the towers with 64-wide heads, ViT and BERT — what the BERT-only kernels are instantiated at (the BERT
// embedding, the post-LN operand sets of the mixed kernel); ROW_WIDTH_SWITCH: those and 1280, for the kernels the ViT executor launches.
#define ROW_WIDTH_SWITCH_64(width, X, A)                                                                                      \
    switch (width) {                                                                                                           \
        case 128: X(128, A); break;                                                                                            \
        case 192: X(192, A); break;                                                                                            \
        case 256: X(256, A); break;                                                                                            \
        case 384: X(384, A); break;                                                                                            \
        case 768: X(768, A); break;                                                                                            \
        default: X(1024, A); break;                                                                                            \
    }
#define ROW_WIDTH_SWITCH(width, X, A)                                                                                         \
    if ((width) == 1280) { X(1280, A); } else ROW_WIDTH_SWITCH_64(width, X, A)

// width: one of the instantiated row widths (anything else is IISAN_EBADSHAPE)
int launch_add2_layernorm768(int dtype16, const float* x, const void* delta16, const void* delta16b, const float* g,
                             const float* b, float eps, float* sum32, void* out16, float* out32, int64_t rows, int width, hipStream_t s,
                             const RowKeep* keep) {
    IISAN_CHECK_SHAPE(row_width_instantiated(width), "layernorm: " ROW_WIDTH_MSG, width);
    if (rows <= 0) return IISAN_OK;
    const int64_t blocks = ceil_div(rows, (int64_t)(256 / row_lpr(width, 4, 64)));       // 4 rows per workgroup from 768 on, up to 16 below
    IISAN_CHECK_SHAPE(blocks < (1ll << 31), "layernorm: grid too large");
    dim3 grid((unsigned)blocks), block(256);
    const int v = (delta16 ? 1 : 0) | (delta16b ? 2 : 0) | (sum32 ? 4 : 0) | (g ? 8 : 0);
#define LN768_LAUNCH(TT, EL, V, W)                                                                                             \
    hipLaunchKernelGGL((layernorm768_kernel<TT, V, W>), grid, block, 0, s, x, (const EL*)delta16, (const EL*)delta16b, g, b, eps, sum32, (EL*)out16, out32, rows)
#define LN768_KEEP(TT, EL)                                                                                                     \
    hipLaunchKernelGGL((layernorm768_kernel<TT, 9, 768, RowKeep>), grid, block, 0, s, x, (const EL*)delta16, (const EL*)delta16b, g, b, eps, sum32, (EL*)out16, out32, rows, *keep)
    if (keep) {         // train mode: x = LN(x + keep * delta16) at 768 or a refusal, never a silent eval launch
        IISAN_CHECK_SHAPE(v == 9 && width == 768, "layernorm: no train-mode instantiation of operand set %d at row width %d", v, width);
        if (dtype16 == IISAN_BF16) LN768_KEEP(BF16, __bf16); else LN768_KEEP(F16, _Float16);
        iisan_count_bert_drop();
        IISAN_LAUNCH_OK();
        return IISAN_OK;
    }
#define LN768_AT(W, V)                                                                                                         \
    if (dtype16 == IISAN_BF16) LN768_LAUNCH(BF16, __bf16, V, W); else LN768_LAUNCH(F16, _Float16, V, W)
#define LN768_CASE(V)                                                                                                          \
    case V:                                                                                                                    \
        ROW_WIDTH_SWITCH(width, LN768_AT, V)                                                                                   \
        break
    switch (v) {
        LN768_CASE(0); LN768_CASE(1); LN768_CASE(2); LN768_CASE(3); LN768_CASE(4); LN768_CASE(5); LN768_CASE(6); LN768_CASE(7);
        LN768_CASE(8); LN768_CASE(9); LN768_CASE(10); LN768_CASE(11); LN768_CASE(12); LN768_CASE(13); LN768_CASE(14); LN768_CASE(15);
    }
#undef LN768_AT
#undef LN768_CASE
#undef LN768_KEEP
#undef LN768_LAUNCH
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}


// mixed-precision residual stream (layernorm768_mixed_kernel): V = MX_* flags of the operands that exist; the operand sets of the
// LayerNorm-image routes exist at every instantiated width, those of the product route (MX_STAT, MX_BLK32) at 768 only
int launch_layernorm768_mixed(int dtype16, int V, const float* x32, void* x16, float* xc, const void* delta16, const void* delta16b,
                              const float* g, const float* b, float eps, void* out16, int64_t items, int Ttok, int width, hipStream_t s,
                              float* stat, const RowKeep* keep) {
    IISAN_CHECK_SHAPE(row_width_instantiated(width), "layernorm768_mixed: " ROW_WIDTH_MSG, width);
    if (items <= 0) return IISAN_OK;
    IISAN_CHECK_SHAPE(!(V & MX_STAT) || stat, "layernorm768_mixed: MX_STAT needs the statistics buffer");
    const int tpw = 256 / row_lpr(width, 8, 32);          // tokens (CLS-only: items) per workgroup: 8 from 768 on, up to 32 below
    const int64_t blocks = (V & MX_CLSONLY) ? ceil_div(items, (int64_t)tpw) : items * ((Ttok + tpw - 1) / tpw);
    IISAN_CHECK_SHAPE(blocks < (1ll << 31), "layernorm768_mixed: grid too large");
    dim3 grid((unsigned)blocks), block(256);
#define MX_LAUNCH(TT, EL, VV, W)                                                                                               \
    hipLaunchKernelGGL((layernorm768_mixed_kernel<TT, VV, W>), grid, block, 0, s, x32, (_Float16*)x16, xc, (const EL*)delta16, (const EL*)delta16b, g, b, eps, (EL*)out16, items, Ttok, stat)
#define MX_KEEP(TT, EL, VV)                                                                                                    \
    hipLaunchKernelGGL((layernorm768_mixed_kernel<TT, VV, 768, RowKeep>), grid, block, 0, s, x32, (_Float16*)x16, xc, (const EL*)delta16, (const EL*)delta16b, g, b, eps, (EL*)out16, items, Ttok, stat, *keep)
    if (keep) {         // train mode: BERT's x = LN(x + keep * d) at 768 or a refusal, never a silent eval launch
        const bool alias = (V & MX_ALIAS) != 0;
        IISAN_CHECK_SHAPE((V & ~MX_ALIAS) == (MX_D1 | MX_LN | MX_RESY) && width == 768,
                          "layernorm768_mixed: no train-mode instantiation of operand set %d at row width %d", V, width);
        IISAN_CHECK_SHAPE(!alias || (dtype16 == IISAN_F16 && out16 == x16), "layernorm768_mixed, train mode: the aliased image needs fp16 operands and out16 == x16");
        if (dtype16 == IISAN_BF16) MX_KEEP(BF16, __bf16, MX_D1 | MX_LN | MX_RESY);
        else if (alias) MX_KEEP(F16, _Float16, MX_D1 | MX_LN | MX_RESY | MX_ALIAS);
        else MX_KEEP(F16, _Float16, MX_D1 | MX_LN | MX_RESY);
        iisan_count_bert_drop();
        IISAN_LAUNCH_OK();
        return IISAN_OK;
    }
#define MX_CASE768(VV)                                                                                                         \
    case VV:                                                                                                                   \
        if (width != 768) break;                                                                                               \
        if (dtype16 == IISAN_BF16) MX_LAUNCH(BF16, __bf16, VV, 768); else MX_LAUNCH(F16, _Float16, VV, 768);                   \
        IISAN_LAUNCH_OK();                                                                                                     \
        return IISAN_OK
#define MX_AT(W, VV)                                                                                                           \
    if (dtype16 == IISAN_BF16) MX_LAUNCH(BF16, __bf16, VV, W); else MX_LAUNCH(F16, _Float16, VV, W)
#define MX_CASE(VV)                                                                                                            \
    case VV:                                                                                                                   \
        ROW_WIDTH_SWITCH(width, MX_AT, VV)                                                                                     \
        IISAN_LAUNCH_OK();                                                                                                     \
        return IISAN_OK
#define MX_CASE_BERT(VV)                                                                                                       \
    case VV:                                                                                                                   \
        if (width == 1280) break;                                                                                              \
        ROW_WIDTH_SWITCH_64(width, MX_AT, VV)                                                                                  \
        IISAN_LAUNCH_OK();                                                                                                     \
        return IISAN_OK
    switch (V) {
        MX_CASE(MX_SRC32 | MX_RESV | MX_LN);               // ViT block 0, LN1: fp32 embeddings -> fp16 stream + LN image
        MX_CASE(MX_SRC32 | MX_POSROW | MX_D1 | MX_RESV | MX_LN);   // ViT block 0, LN1: position table + 16-bit patch embedding -> stream + image
        MX_CASE(MX_D1 | MX_LN);                            // ViT LN2: LN(x + dO), x not written
        MX_CASE(MX_D1 | MX_D2 | MX_RESV | MX_LN);          // ViT LN1: x += dO + dF; LN
        MX_CASE(MX_D1 | MX_D2 | MX_RESV | MX_CLSONLY);     // ViT closing add of the CLS rows (the last hidden state)
        MX_CASE_BERT(MX_D1 | MX_LN | MX_RESY);             // BERT: x = LN(x + d) (no BERT is 1280 wide)
        MX_CASE_BERT(MX_D1 | MX_LN | MX_RESY | MX_ALIAS);  // BERT, fp16 operands: ... and the image IS the stream
        // LayerNorm applied by the consuming product (Gemm16Args::rowstat): the stream and the row statistics only — 768 wide
        MX_CASE768(MX_SRC32 | MX_POSROW | MX_D1 | MX_RESV | MX_STAT);   // ViT block 0
        MX_CASE768(MX_SRC32 | MX_POSROW | MX_D1 | MX_RESV | MX_STAT | MX_BLK32);   // ... into a block-major stream
        MX_CASE768(MX_D1 | MX_RESV | MX_STAT);             // ViT LN1 (x += dF) and LN2 (x += dO)
        MX_CASE768(MX_D1 | MX_RESV | MX_CLSONLY);          // ViT closing add of the CLS rows when x + dO is in the stream already
        default: break;
    }
#undef MX_AT
#undef MX_CASE
#undef MX_CASE_BERT
#undef MX_CASE768
#undef MX_KEEP
#undef MX_LAUNCH
    iisan_set_error("layernorm768_mixed: operand set %d not instantiated at row width %d", V, width);
    return IISAN_EBADSHAPE;
}

// the opening step of a CLIP tower (clip_open_kernel): every instantiated width, both operand types
int launch_clip_open(int dtype16, const float* pos, void* x16, float* xc, const void* patch16, const float* pre_g, const float* pre_b,
                     const float* g, const float* b, float eps, void* out16, int64_t items, int Ttok, int width, hipStream_t s) {
    IISAN_CHECK_SHAPE(row_width_instantiated(width), "clip_open: " ROW_WIDTH_MSG, width);
    IISAN_CHECK_SHAPE(pre_g && pre_b && g && b, "clip_open: null LayerNorm weights");
    if (items <= 0) return IISAN_OK;
    const int tpw = 256 / row_lpr(width, 8, 32);
    const int64_t blocks = items * ((Ttok + tpw - 1) / tpw);
    IISAN_CHECK_SHAPE(blocks < (1ll << 31), "clip_open: grid too large");
    dim3 grid((unsigned)blocks), block(256);
#define CLIP_OPEN_AT(W, A)                                                                                                     \
    if (dtype16 == IISAN_BF16)                                                                                                 \
        hipLaunchKernelGGL((clip_open_kernel<BF16, W>), grid, block, 0, s, pos, (_Float16*)x16, xc, (const __bf16*)patch16, pre_g, pre_b, g, b, eps, (__bf16*)out16, items, Ttok); \
    else                                                                                                                       \
        hipLaunchKernelGGL((clip_open_kernel<F16, W>), grid, block, 0, s, pos, (_Float16*)x16, xc, (const _Float16*)patch16, pre_g, pre_b, g, b, eps, (_Float16*)out16, items, Ttok)
    ROW_WIDTH_SWITCH(width, CLIP_OPEN_AT, 0)
#undef CLIP_OPEN_AT
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_add_layernorm768(int dtype16, const float* x, const void* delta16, const float* g, const float* b, float eps,
                            float* sum32, void* out16, float* out32, int64_t rows, int width, hipStream_t s, const RowKeep* keep) {
    return launch_add2_layernorm768(dtype16, x, delta16, nullptr, g, b, eps, sum32, out16, out32, rows, width, s, keep);
}

int launch_layernorm768(int dtype16, const float* x, const float* g, const float* b, float eps, void* out16,
                        float* out32, int64_t rows, int width, hipStream_t s) {
    return launch_add_layernorm768(dtype16, x, nullptr, g, b, eps, nullptr, out16, out32, rows, width, s);
}

// columns of a patch row in the patch matrix (and of a row of the packed patch weight): C p p, zero-padded to a multiple of 64 where the
// patch side is no multiple of 8
int vit_patch_ld(int C, int p) { return p % 8 == 0 ? C * p * p : (int)ceil_div(C * p * p, 64) * 64; }

// The uint8 patch extraction with per-channel statistics (norm = mean[3] | std[3], host): direct (index == null) or indexed
static int vit_im2col_norm(int dtype16, const uint8_t* img, int64_t rows, const int64_t* index, void* out, int64_t M, int C, int R, int p,
                           const float* norm, hipStream_t s) {
    IISAN_CHECK_SHAPE(C == 3, "vit: per-channel normalisation statistics are given for 3 channels, the tower has %d", C);
    IISAN_CHECK_SHAPE(norm[3] != 0.f && norm[4] != 0.f && norm[5] != 0.f, "vit: norm_std (%g, %g, %g) must be non-zero where norm_mean / norm_std are set",
                      (double)norm[3], (double)norm[4], (double)norm[5]);
    const PixNorm nrm{{norm[0], norm[1], norm[2]}, {norm[3], norm[4], norm[5]}};
    const int ldp = vit_patch_ld(C, p);
    const int64_t total = M * (R / p) * (R / p) * (ldp / 8);
    const unsigned grid = (unsigned)(ceil_div(total, 256) < 262144 ? ceil_div(total, 256) : 262144);
#define IM2COL_NORM(TT, EL, IDX)                                                                                               \
    if (p % 8 != 0) hipLaunchKernelGGL((vit_im2col_pad_kernel<TT, uint8_t, IDX, PixNorm>), dim3(grid), dim3(256), 0, s, img, (EL*)out, M, C, R, p, ldp, index, rows, nrm); \
    else hipLaunchKernelGGL((vit_im2col_kernel<TT, uint8_t, IDX, PixNorm>), dim3(grid), dim3(256), 0, s, img, (EL*)out, M, C, R, p, index, rows, nrm)
    if (index) {
        if (dtype16 == IISAN_BF16) { IM2COL_NORM(BF16, __bf16, true); } else { IM2COL_NORM(F16, _Float16, true); }
    } else {
        if (dtype16 == IISAN_BF16) { IM2COL_NORM(BF16, __bf16, false); } else { IM2COL_NORM(F16, _Float16, false); }
    }
#undef IM2COL_NORM
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_vit_im2col(int dtype16, const void* img, int img_u8, void* out, int64_t M, int C, int R, int p, hipStream_t s, const float* norm) {
    if (norm && img_u8) return vit_im2col_norm(dtype16, (const uint8_t*)img, 0, nullptr, out, M, C, R, p, norm, s);
    if (p % 8 != 0) {
        const int ldp = vit_patch_ld(C, p);
        const int64_t total = M * (R / p) * (R / p) * (ldp / 8);
        const unsigned grid = (unsigned)(ceil_div(total, 256) < 262144 ? ceil_div(total, 256) : 262144);
        if (img_u8) {
            if (dtype16 == IISAN_BF16)
                hipLaunchKernelGGL((vit_im2col_pad_kernel<BF16, uint8_t>), dim3(grid), dim3(256), 0, s, (const uint8_t*)img, (__bf16*)out, M, C, R, p, ldp);
            else
                hipLaunchKernelGGL((vit_im2col_pad_kernel<F16, uint8_t>), dim3(grid), dim3(256), 0, s, (const uint8_t*)img, (_Float16*)out, M, C, R, p, ldp);
        } else {
            if (dtype16 == IISAN_BF16)
                hipLaunchKernelGGL((vit_im2col_pad_kernel<BF16, float>), dim3(grid), dim3(256), 0, s, (const float*)img, (__bf16*)out, M, C, R, p, ldp);
            else
                hipLaunchKernelGGL((vit_im2col_pad_kernel<F16, float>), dim3(grid), dim3(256), 0, s, (const float*)img, (_Float16*)out, M, C, R, p, ldp);
        }
        IISAN_LAUNCH_OK();
        return IISAN_OK;
    }
    const int64_t total = M * (R / p) * (R / p) * (C * p * p / 8);
    const unsigned grid = (unsigned)(ceil_div(total, 256) < 262144 ? ceil_div(total, 256) : 262144);
    if (img_u8) {
        if (dtype16 == IISAN_BF16)
            hipLaunchKernelGGL((vit_im2col_kernel<BF16, uint8_t>), dim3(grid), dim3(256), 0, s, (const uint8_t*)img, (__bf16*)out, M, C, R, p);
        else
            hipLaunchKernelGGL((vit_im2col_kernel<F16, uint8_t>), dim3(grid), dim3(256), 0, s, (const uint8_t*)img, (_Float16*)out, M, C, R, p);
    } else {
        if (dtype16 == IISAN_BF16)
            hipLaunchKernelGGL((vit_im2col_kernel<BF16, float>), dim3(grid), dim3(256), 0, s, (const float*)img, (__bf16*)out, M, C, R, p);
        else
            hipLaunchKernelGGL((vit_im2col_kernel<F16, float>), dim3(grid), dim3(256), 0, s, (const float*)img, (_Float16*)out, M, C, R, p);
    }
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_vit_im2col_indexed(int dtype16, const uint8_t* catalogue, int64_t rows, const int64_t* index, void* out, int64_t M, int C,
                              int R, int p, hipStream_t s, const float* norm) {
    if (norm) return vit_im2col_norm(dtype16, catalogue, rows, index, out, M, C, R, p, norm, s);
    if (p % 8 != 0) {
        const int ldp = vit_patch_ld(C, p);
        const int64_t total = M * (R / p) * (R / p) * (ldp / 8);
        const unsigned grid = (unsigned)(ceil_div(total, 256) < 262144 ? ceil_div(total, 256) : 262144);
        if (dtype16 == IISAN_BF16)
            hipLaunchKernelGGL((vit_im2col_pad_kernel<BF16, uint8_t, true>), dim3(grid), dim3(256), 0, s, catalogue, (__bf16*)out, M, C, R, p, ldp, index, rows);
        else
            hipLaunchKernelGGL((vit_im2col_pad_kernel<F16, uint8_t, true>), dim3(grid), dim3(256), 0, s, catalogue, (_Float16*)out, M, C, R, p, ldp, index, rows);
        IISAN_LAUNCH_OK();
        return IISAN_OK;
    }
    const int64_t total = M * (R / p) * (R / p) * (C * p * p / 8);
    const unsigned grid = (unsigned)(ceil_div(total, 256) < 262144 ? ceil_div(total, 256) : 262144);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL((vit_im2col_kernel<BF16, uint8_t, true>), dim3(grid), dim3(256), 0, s, catalogue, (__bf16*)out, M, C, R, p, index, rows);
    else
        hipLaunchKernelGGL((vit_im2col_kernel<F16, uint8_t, true>), dim3(grid), dim3(256), 0, s, catalogue, (_Float16*)out, M, C, R, p, index, rows);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_vit_cls_rows(float* X, const float* cls, const float* pos, int64_t M, int T, int D, hipStream_t s) {
    hipLaunchKernelGGL(vit_cls_rows_kernel, dim3((unsigned)ceil_div(M * D, 256)), dim3(256), 0, s, X, cls, pos, M, T, D);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

// one launcher for the direct (index == null) and the indexed form; width: one of the instantiated row widths
template <bool IDX>
static int bert_embed_ln_any(int dtype16, const int64_t* text, int64_t rows, const int64_t* index, const float* word, const float* pos,
                             const float* type0, const float* g, const float* b, float eps, float* X, void* H, float* key_bias,
                             int64_t M, int W, int vocab, int width, hipStream_t s, void* X16, float* Xc, const RowKeep* keep) {
    IISAN_CHECK_SHAPE(row_width_instantiated(width) && width != 1280, "bert_embed_ln: " ROW_WIDTH_MSG " — 1280 on the ViT's kernels only", width);
    dim3 grid((unsigned)ceil_div(M * W, (int64_t)(256 / row_lpr(width, 4, 64)))), block(256);
#define EMBED_LAUNCH(TT, EL, WD)                                                                                               \
    hipLaunchKernelGGL((bert_embed_ln_kernel<TT, IDX, WD>), grid, block, 0, s, text, word, pos, type0, g, b, eps, X, (EL*)H, key_bias, M, W, vocab, (_Float16*)X16, Xc, index, rows)
#define EMBED_KEEP(TT, EL)                                                                                                     \
    hipLaunchKernelGGL((bert_embed_ln_kernel<TT, IDX, 768, RowKeep>), grid, block, 0, s, text, word, pos, type0, g, b, eps, X, (EL*)H, key_bias, M, W, vocab, (_Float16*)X16, Xc, index, rows, *keep)
#define EMBED_DEB(TT, EL, WD)                                                                                                  \
    hipLaunchKernelGGL((bert_embed_ln_kernel<TT, IDX, WD, RowKeepDeberta>), grid, block, 0, s, text, word, pos, type0, g, b, eps, X, (EL*)H, key_bias, M, W, vocab, (_Float16*)X16, Xc, index, rows)
    IISAN_CHECK_SHAPE(!pos == !type0, "bert_embed_ln: the position and the type table come together (BERT) or not at all (DeBERTa)");
    if (!pos) {         // DeBERTa: eval mode only
        IISAN_CHECK_SHAPE(!keep, "bert_embed_ln: no train-mode instantiation of the DeBERTa embedding step");
#define EMBED_DEB_AT(WD, TT)                                                                                                   \
    if (dtype16 == IISAN_BF16) EMBED_DEB(BF16, __bf16, WD); else EMBED_DEB(TT, _Float16, WD)
        ROW_WIDTH_SWITCH_64(width, EMBED_DEB_AT, F16)
#undef EMBED_DEB_AT
    } else if (keep) {         // train mode: 768 or a refusal, never a silent eval launch
        IISAN_CHECK_SHAPE(width == 768, "bert_embed_ln: no train-mode instantiation at row width %d", width);
        if (dtype16 == IISAN_BF16) EMBED_KEEP(BF16, __bf16); else EMBED_KEEP(F16, _Float16);
        iisan_count_bert_drop();
    } else {
#define EMBED_AT(WD, TT)                                                                                                       \
    if (dtype16 == IISAN_BF16) EMBED_LAUNCH(BF16, __bf16, WD); else EMBED_LAUNCH(TT, _Float16, WD)
        ROW_WIDTH_SWITCH_64(width, EMBED_AT, F16)
#undef EMBED_AT
    }
#undef EMBED_DEB
#undef EMBED_KEEP
#undef EMBED_LAUNCH
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_bert_embed_ln(int dtype16, const int64_t* text, const float* word, const float* pos, const float* type0,
                         const float* g, const float* b, float eps, float* X, void* H, float* key_bias, int64_t M,
                         int W, int vocab, int width, hipStream_t s, void* X16, float* Xc, const RowKeep* keep) {       // X == null: mixed stream (X16 + Xc)
    return bert_embed_ln_any<false>(dtype16, text, 0, nullptr, word, pos, type0, g, b, eps, X, H, key_bias, M, W, vocab, width, s, X16, Xc, keep);
}

int launch_bert_embed_ln_indexed(int dtype16, const int64_t* table, int64_t rows, const int64_t* index, const float* word, const float* pos,
                                 const float* type0, const float* g, const float* b, float eps, float* X, void* H, float* key_bias,
                                 int64_t M, int W, int vocab, int width, hipStream_t s, void* X16, float* Xc, const RowKeep* keep) {
    return bert_embed_ln_any<true>(dtype16, table, rows, index, word, pos, type0, g, b, eps, X, H, key_bias, M, W, vocab, width, s, X16, Xc, keep);
}

int launch_gather_rows16(const void* H, void* out, int64_t M, int T, int D, hipStream_t s) {
    const int D8 = D / 8;
    hipLaunchKernelGGL(gather_rows16_kernel, dim3((unsigned)ceil_div(M * D8, 256)), dim3(256), 0, s, (const uint4*)H, (uint4*)out, M, T, D8);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_gather_cls(const float* X, float* taps, int64_t M, int T, int D, int n_taps, int k, hipStream_t s) {
    hipLaunchKernelGGL(gather_cls_kernel, dim3((unsigned)ceil_div(M * (D / 4), 256)), dim3(256), 0, s, X, taps, M, T, D, n_taps, k);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_layernorm768(int32_t dtype16, const float* x, const float* g, const float* b, float eps,
                                  void* out16, float* out32, int64_t rows, void* stream) {
    return launch_layernorm768(dtype16, x, g, b, eps, out16, out32, rows, 768, (hipStream_t)stream);
}

extern "C" int iisan_layernorm(int32_t dtype16, const float* x, const float* g, const float* b, float eps,
                               void* out16, float* out32, int64_t rows, int32_t width, void* stream) {
    return launch_layernorm768(dtype16, x, g, b, eps, out16, out32, rows, width, (hipStream_t)stream);
}

// ---- packed tap store gather: out[m, :] = fp32(table[ids[m], :]), rows of `row_elems` (multiple of 8) ----
// one thread = 8 consecutive elements (16-B loads from a 16-bit store, 2x16-B from an fp32 one; two 16-B stores)
template <typename TS>
__global__ __launch_bounds__(256) void gather_taps_kernel(const TS* __restrict__ table, const int64_t* __restrict__ ids,
                                                          float* __restrict__ out, int64_t M, int64_t row_elems, int64_t rows) {
    const int64_t per_row = row_elems / 8;
    const int64_t total = M * per_row;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = i / per_row, c = (i - m * per_row) * 8;
        int64_t id = ids[m];
        id = id < 0 ? 0 : (id >= rows ? rows - 1 : id);
        const TS* src = table + id * row_elems + c;
        f4 lo, hi;
        if constexpr (sizeof(TS) == 4) {
            lo = *(const f4*)src;
            hi = *(const f4*)(src + 4);
        } else {
            typedef TS V8 __attribute__((ext_vector_type(8)));
            const V8 v = *(const V8*)src;
#pragma unroll
            for (int e = 0; e < 4; ++e) { lo[e] = (float)v[e]; hi[e] = (float)v[4 + e]; }
        }
        *(f4*)(out + m * row_elems + c) = lo;
        *(f4*)(out + m * row_elems + c + 4) = hi;
    }
}

extern "C" int iisan_gather_taps(int32_t store_dtype, const void* table, int64_t rows, const int64_t* ids, float* out,
                                 int64_t M, int64_t row_elems, void* stream) {
    if (M <= 0) return IISAN_OK;
    IISAN_CHECK_SHAPE(row_elems > 0 && row_elems % 8 == 0 && rows > 0, "gather_taps: row length %lld must be a positive multiple of 8", (long long)row_elems);
    const int64_t total = M * (row_elems / 8);
    const unsigned grid = (unsigned)(ceil_div(total, 256) < 262144 ? ceil_div(total, 256) : 262144);
    hipStream_t s = (hipStream_t)stream;
    if (store_dtype == IISAN_F32)
        hipLaunchKernelGGL(gather_taps_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)table, ids, out, M, row_elems, rows);
    else if (store_dtype == IISAN_BF16)
        hipLaunchKernelGGL(gather_taps_kernel<__bf16>, dim3(grid), dim3(256), 0, s, (const __bf16*)table, ids, out, M, row_elems, rows);
    else if (store_dtype == IISAN_F16)
        hipLaunchKernelGGL(gather_taps_kernel<_Float16>, dim3(grid), dim3(256), 0, s, (const _Float16*)table, ids, out, M, row_elems, rows);
    else {
        iisan_set_error("gather_taps: unknown store dtype %d", store_dtype);
        return IISAN_EBADSHAPE;
    }
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_cast16(int32_t dtype16, const float* src, void* dst, int64_t n, void* stream) {
    if (n <= 0) return IISAN_OK;
    const unsigned grid = (unsigned)(ceil_div(n, 256) < 65536 ? ceil_div(n, 256) : 65536);
    if (dtype16 == IISAN_BF16)
        hipLaunchKernelGGL(cast16_kernel<BF16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (__bf16*)dst, n);
    else
        hipLaunchKernelGGL(cast16_kernel<F16>, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, (_Float16*)dst, n);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

// ---- LayerNorm folded into the weights of the product that consumes it (Gemm16Args::rowstat) ----
// LN(x) W^T + b = rstd (x Wf^T) + bf with Wf[n][k] = gamma[k] W[n][k] - (1/K) sum_j gamma[j] W[n][j] — CENTRED rows: sum_k x[k] Wf[n][k] =
// sum_k (x[k] - mean(x)) gamma[k] W[n][k] for every x, so the product of the un-normalised row needs no mean correction — and
// bf = b + W beta.  The fp16 rounding of Wf leaves a row sum d_n = sum_k (Wf16 - Wf) != 0 and with it an error mean(x) rstd d_n that
// grows with |mean| / std of the row (CPU emulation: 1.7e-4 -> 5.1e-4 relative at |mean| = 3 std with round-to-nearest, |d_n| ~ 8 ulp).
// SUM-PRESERVING ROUNDING: round to nearest, then move the few elements whose rounding was the closest call (residual nearest +-1/2
// ulp, on the side d_n needs) to their other neighbour — a bisection over the residual threshold finds the set whose ulps add up to
// d_n; each such move costs next to nothing ((1 - 2|r|) ulp^2 of squared error at residual r ~ 1/2), so the weights keep the noise of
// plain rounding (the first version diffused every element's error into its neighbour: row sums as good, 1.4 x the noise) — and what
// the bisection leaves (< one ulp) goes into one element.  |d_n| ends below one ulp of one weight, ~1e-5 of the ~4e-4 plain rounding
// leaves.  W is read from the caller's fp32 master when the weights struct has one (iisan_layer_weights.qkv_w32 / fc1_w32): ONE rounding
// of gamma W - mean instead of a second one on top of the 16-bit copy's.  The weights are frozen, but the ABI is stateless: folded once
// per forward call (200-300 MB of traffic for ViT-B, ~40-60 us) into the workspace.
// Half a wave per weight row (K = 768: three 8-element pieces per lane), 8 rows per workgroup, every job in one launch.
struct LnFoldArgs { LnFoldJob j[32]; int32_t row0[33]; int32_t n; };

__global__ __launch_bounds__(256) void fold_ln_weights_kernel(LnFoldArgs a) {
    const int lane = threadIdx.x & 31;
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5);
    if (row >= a.row0[a.n]) return;
    int ji = 0;
    while (row >= a.row0[ji + 1]) ++ji;
    const LnFoldJob& J = a.j[ji];
    const int n = row - a.row0[ji];
    _Float16* wf = (_Float16*)J.Wf + (int64_t)n * 768;
    auto sum32 = [](float t) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        return t;
    };
    float v[3][8];
    float cs = 0.f, bw = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 8;
        float x[8];
        if (J.w32) {
            const float* w = (const float*)J.W + (int64_t)n * 768 + c;
            const f4 x0 = *(const f4*)w, x1 = *(const f4*)(w + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { x[e] = x0[e]; x[4 + e] = x1[e]; }
        } else {
            const h8 xh = *(const h8*)((const _Float16*)J.W + (int64_t)n * 768 + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (float)xh[e];
        }
        const f4 g0 = *(const f4*)(J.g + c), g1 = *(const f4*)(J.g + c + 4), b0 = *(const f4*)(J.b + c), b1 = *(const f4*)(J.b + c + 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] = x[e] * (e < 4 ? g0[e] : g1[e - 4]);
            cs += v[i][e];
            bw += x[e] * (e < 4 ? b0[e] : b1[e - 4]);
        }
    }
    cs = sum32(cs); bw = sum32(bw);
    const float mu = cs * (1.0f / 768.0f);
    // round to nearest; r = residual in units of the element's OWN ulp towards the side the row sum needs (dir = sign of the total residual)
    _Float16 o[3][8];
    float res = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] -= mu;
            o[i][e] = (_Float16)v[i][e];
            res += v[i][e] - (float)o[i][e];
        }
    const float R = sum32(res);                       // what the emitted row is short of (target - emitted)
    const float dir = R >= 0.f ? 1.f : -1.f;
    // the neighbour of o on the `dir` side and what moving there adds to the row sum (its ulp on that side)
    float step[3][8], frac[3][8];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float of = (float)o[i][e];
            const unsigned short bits = __builtin_bit_cast(unsigned short, o[i][e]);
            // next representable half away from / towards zero: +-1 on the magnitude bits (zero: the smallest subnormal of sign dir)
            const bool up_mag = (of > 0.f) == (dir > 0.f) || of == 0.f;
            unsigned short nb = of == 0.f ? (unsigned short)(dir > 0.f ? 1 : 0x8001) : (unsigned short)(up_mag ? bits + 1 : bits - 1);
            const float nf = (float)__builtin_bit_cast(_Float16, nb);
            step[i][e] = (nf - of) * dir;                                    // > 0
            frac[i][e] = (v[i][e] - of) * dir / step[i][e];                  // in [-1/2, 1/2]: how far the target lies towards that neighbour
        }
    // bisection over the threshold t: move every element with frac > t; moved(t) decreases from ~sum of all steps (t = -1/2) to 0 (t = 1/2)
    float lo = 0.f, hi = 0.5f;                        // elements with frac <= 0 were rounded away from that side: never moved
    const float need = R * dir;                       // >= 0
#pragma unroll 1
    for (int it = 0; it < 12; ++it) {
        const float t = 0.5f * (lo + hi);
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) m += frac[i][e] > t ? step[i][e] : 0.f;
        m = sum32(m);
        if (m > need) lo = t; else hi = t;            // too much moved: raise the threshold
    }
    float moved = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (frac[i][e] > hi) {
                o[i][e] = (_Float16)((float)o[i][e] + dir * step[i][e]);
                moved += step[i][e];
            }
    const float rest = (need - sum32(moved)) * dir;   // |rest| < one ulp of the last element not moved: into one element, re-rounded
    if (lane == 0) o[0][0] = (_Float16)((float)o[0][0] + rest);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        h8 o8;
#pragma unroll
        for (int e = 0; e < 8; ++e) o8[e] = o[i][e];
        *(h8*)(wf + i * 256 + lane * 8) = o8;
    }
    if (lane == 0) J.bf[n] = (J.bias ? J.bias[n] : 0.f) + bw;
}

int launch_fold_ln_weights(const LnFoldJob* jobs, int n, hipStream_t s) {
    IISAN_CHECK_SHAPE(n >= 0 && n <= 32, "fold_ln_weights: %d jobs (at most 32 per launch)", n);
    if (n == 0) return IISAN_OK;
    LnFoldArgs a{};
    a.n = n;
    for (int i = 0; i < n; ++i) { a.j[i] = jobs[i]; a.row0[i + 1] = a.row0[i] + jobs[i].N; }
    hipLaunchKernelGGL(fold_ln_weights_kernel, dim3((unsigned)ceil_div((int64_t)a.row0[n], 8)), dim3(256), 0, s, a);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

// ---- after an EPI_STREAM16 product (gemm16_h256.hip): the rows' rstd from the per-slice partial sums, and the CLS rows ----
// Blocks [0, ceil(rows / 256)): one thread per row sums the `nslots` (sum, sum of squares) pairs in slice order — a fixed order, so the
// statistics are bit-reproducible — and writes rstd; single-pass variance in fp32 (E[x^2] - mean^2: the stream's rows have |mean| well
// under their spread; relative error ~1e-7 (1 + mean^2 / var)).  CLS rows are skipped there and done by the blocks behind: half a wave
// per item adds the fp16 delta the product left in the stream's CLS slot to the item's fp32 stream, writes the rounded sum back (the
// next product's A operand) and the rstd of the ROUNDED row, two-pass.
__global__ __launch_bounds__(256) void stream_stats_finalize_kernel(const f2* __restrict__ part, int nslots, int64_t Mpad, _Float16* x16,
                                                                    float* xc, float* __restrict__ rstat, float eps, int64_t items,
                                                                    int Ttok, unsigned row_blocks, int x16_blk32) {
    const int64_t rows = items * Ttok;
    if (blockIdx.x < row_blocks) {
        const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (row >= rows || row % Ttok == 0) return;
        float s = 0.f, q = 0.f;
        if (nslots == 12) {
            // D = 768: all twelve slice partials requested at once, same summation order, same bits (round 5; no measurable change —
            // 8.2 - 10.3 us per launch either way: the launch is its boundary + the CLS blocks, not this loop)
            f2 v[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) v[j] = part[(int64_t)j * Mpad + row];
#pragma unroll
            for (int j = 0; j < 12; ++j) { s += v[j][0]; q += v[j][1]; }
        } else {
            for (int j = 0; j < nslots; ++j) {
                const f2 v = part[(int64_t)j * Mpad + row];
                s += v[0]; q += v[1];
            }
        }
        const float mean = s * (1.0f / 768.0f);
        const float var = fmaxf(q * (1.0f / 768.0f) - mean * mean, 0.f);
        rstat[row] = rsqrtf(var + eps);
        return;
    }
    const int lane = threadIdx.x & 31;
    const int64_t item = (int64_t)(blockIdx.x - row_blocks) * 8 + (threadIdx.x >> 5);
    if (item >= items) return;
    const int64_t row = item * Ttok;
    float v[3][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = i * 256 + lane * 8;
        // (block-major stream: the lane's 8 columns are one 16-byte granule of it, common.h)
        _Float16* xp = x16 + (x16_blk32 ? blk32_byte(row, c, 768) >> 1 : row * 768 + c);
        const h8 d = *(const h8*)xp;
        const f4 a = *(const f4*)(xc + item * 768 + c), b = *(const f4*)(xc + item * 768 + c + 4);
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            v[i][e] = (e < 4 ? a[e] : b[e - 4]) + (float)d[e];
            o[e] = (_Float16)v[i][e];
        }
        *(f4*)(xc + item * 768 + c) = (f4){v[i][0], v[i][1], v[i][2], v[i][3]};
        *(f4*)(xc + item * 768 + c + 4) = (f4){v[i][4], v[i][5], v[i][6], v[i][7]};
        *(h8*)xp = o;
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = (float)o[e]; s += v[i][e]; }
    }
    auto sum32 = [](float t) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        return t;
    };
    const float mean = sum32(s) * (1.0f / 768.0f);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; q += d * d; }
    const float rstd = rsqrtf(sum32(q) * (1.0f / 768.0f) + eps);
    if (lane == 0) rstat[row] = rstd;
}

int launch_stream_stats_finalize(const float* rowpart, int nslots, int64_t Mpad, void* x16, float* xc, float* rstat, float eps,
                                 int64_t items, int Ttok, hipStream_t s, bool x16_blk32) {
    if (items <= 0) return IISAN_OK;
    const int64_t row_blocks = ceil_div(items * Ttok, 256), cls_blocks = ceil_div(items, 8);
    IISAN_CHECK_SHAPE(row_blocks + cls_blocks < (1ll << 31), "stream_stats_finalize: grid too large");
    hipLaunchKernelGGL(stream_stats_finalize_kernel, dim3((unsigned)(row_blocks + cls_blocks)), dim3(256), 0, s, (const f2*)rowpart, nslots, Mpad,
                       (_Float16*)x16, xc, rstat, eps, items, Ttok, (unsigned)row_blocks, x16_blk32 ? 1 : 0);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}
