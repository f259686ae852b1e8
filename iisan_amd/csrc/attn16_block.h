// The per-block arithmetic the three MFMA attention kernels share (device only):
//   attention16_kernel (attn16.hip), attention16_dma_kernel (attn16_dma.hip), attention16_drop_kernel (bert_drop.hip);
//   the streaming-softmax body (attn16_stream.h: one chunk walk behind attention16_long_kernel, attn16_long.hip, and attention16_hd80_kernel,
//   attn16_hd80.hip: 80-wide heads) runs the same pieces per 128-key chunk, with the chunk form of the row softmax below.
// A block = 16 queries of one (item, head) in one wave.  Scores are computed TRANSPOSED, S^T = K · Q^T, on v_mfma_f32_16x16x32: a lane
// (j = lane & 15, g = lane >> 4) holds, for ONE query j, keys 16 t + 4 g + r of score tile t in sc[t][r] — so the softmax row reduction is a
// per-lane loop plus two xor-shuffles (16, 32), and the exponentiated registers are ALREADY in B-operand layout for O^T = V^T · P^T.
// The kernels differ in how Q, K and V travel and in what multiplies P; the fp32 operations below, and their ORDER, are the same for all
// three: bert_drop.hip equals attention16_kernel bit for bit at p = 0, and the two ViT routes are tested against each other.
#pragma once
#include <type_traits>

#include "common.h"

// masked keys carry this RAW score (before the log2(e)/8 scaling): every real score is absorbed by it, like HF's
// additive fp32-min mask, and MASK_RAW * c2 stays finite
constexpr float MASK_RAW = -0x1p126f;      // a power of two: MASK_RAW * c2 is exact, so the fused scale-and-shift below is exactly 0 on all-masked rows
// exp(s/8 - m) = exp2(acc * c2 - m2),  c2 = log2(e) / 8
constexpr float ATTN_C2 = 0.18033688011112042f;

// 16-key tail product of an odd tile count (ViT: 13 tiles): v_mfma_f32_16x16x16 with 4 contraction slots per lane (key base + 4 g + e)
// — no zero-filled half step, no LDS for it
template <typename T> struct Mfma16k16;
template <> struct Mfma16k16<F16> {
    static __device__ __forceinline__ f4 run(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma16k16<BF16> {
    typedef short s4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f4 run(b4 a, b4 b, f4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s4, a), __builtin_bit_cast(s4, b), c, 0, 0, 0);
    }
};

// ---- key limits ----------------------------------------------------------------------------------------------------------------------
// per-key upper limit of the raw score, the value of sKB[r]: +inf keeps, MASK_RAW replaces (a masked key: key_bias < 0; every real score
// is above it), -inf removes a structural pad slot (r >= S)
__device__ __forceinline__ float attn_key_limit(const float* key_bias, int item, int S, int r) {
    return r >= S ? -INFINITY : ((key_bias && key_bias[(int64_t)item * S + r] < 0.f) ? MASK_RAW : INFINITY);
}

// min(score, limit) as ONE instruction the compiler can see — med3(score, limit, -inf).  (fminf() adds two canonicalising v_max; rounds
// 2-4 used an inline-asm v_min_f32 here, which was only safe because a branch stood between it and the MFMAs: the hazard recognizer does
// not look inside inline asm, and with the per-tile branches gone (round 5) the v_min read its MFMA result before the matrix pipe had
// written it — 12 of 18 attention cases wrong.)
__device__ __forceinline__ void attn_apply_key_limit(f4& sc, const f4& lim) {
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = __builtin_amdgcn_fmed3f(sc[r], lim[r], -INFINITY);
}

// ---- row softmax ---------------------------------------------------------------------------------------------------------------------
struct AttnKeepAll {};          // the Keep of the eval-mode kernels: P goes into the P.V product as it is, no multiply is emitted

// sc (raw, limited scores of one query row) becomes p * keep(t, r) with p = exp(s/8 - max), keep(t, r) = the factor of key 16 t + 4 g + r
// (train-mode dropout; AttnKeepAll: 1); returns 1 / (row sum of the UNDROPPED, unrounded p).
// VALU diet (PMC: the eval kernel is VALU-bound, 1088 VALU instructions per 16-query block before): scale+subtract is one fma, and exp2
// is the bare v_exp_f32 (arguments <= 0, results in [0,1]: no range fix-up needed).
// (round 5: two independent max chains and four independent sum chains instead of one 26-deep v_max3 chain and one 52-deep v_add chain —
//  the dependent-issue latency of those chains was exposed time, not arithmetic)
template <int NT16, class Keep>
__device__ __forceinline__ float attn_row_softmax(f4 (&sc)[NT16], Keep keep) {
    float mx0 = -INFINITY, mx1 = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        if (t & 1) mx1 = fmaxf(fmaxf(mx1, sc[t][0]), fmaxf(sc[t][1], fmaxf(sc[t][2], sc[t][3])));
        else mx0 = fmaxf(fmaxf(mx0, sc[t][0]), fmaxf(sc[t][1], fmaxf(sc[t][2], sc[t][3])));
    }
    float mx = fmaxf(mx0, mx1);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    f4 sum4 = {0.f, 0.f, 0.f, 0.f};
    const float mxs = -(mx * ATTN_C2);
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = fmaf(sc[t][r], ATTN_C2, mxs);   // one instruction.  At the maximum the result is the rounding residue of mx*c2
                                                            // (<= 1e-6 in magnitude: exp2 = 1 +- 7e-7), and it is exactly 0 on all-masked
                                                            // rows because MASK_RAW is a power of two
            const float p = __builtin_amdgcn_exp2f(a);      // (a run-time debug select here cost one v_cndmask per score)
            sum4[r] += p;
            if constexpr (std::is_same<Keep, AttnKeepAll>::value) sc[t][r] = p;
            else sc[t][r] = p * keep(t, r);
        }
    float sum = (sum4[0] + sum4[1]) + (sum4[2] + sum4[3]);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    return 1.0f / sum;
}

// Chunk form of attn_row_softmax (the streaming-softmax body, attn16_stream.h; c2 = log2(e) / sqrt(head width)): sc (raw, limited scores of one query row over ONE chunk) becomes p = exp2(sc c2 - ms_new) with
// ms_new = max(ms_old, c2 * chunk maximum); returns ms_new and the chunk's row sum of the unrounded p.  Same instruction diet as the row
// form: two max chains, four sum chains, one fma and the bare v_exp_f32 per score.
struct AttnChunkStat { float ms, sum; };
template <int NT16>
__device__ __forceinline__ AttnChunkStat attn_chunk_softmax(f4 (&sc)[NT16], float ms_old, const float c2 = ATTN_C2) {
    float mx0 = -INFINITY, mx1 = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        if (t & 1) mx1 = fmaxf(fmaxf(mx1, sc[t][0]), fmaxf(sc[t][1], fmaxf(sc[t][2], sc[t][3])));
        else mx0 = fmaxf(fmaxf(mx0, sc[t][0]), fmaxf(sc[t][1], fmaxf(sc[t][2], sc[t][3])));
    }
    float mx = fmaxf(mx0, mx1);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float ms = fmaxf(ms_old, mx * c2);
    const float mxs = -ms;
    f4 sum4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(sc[t][r], c2, mxs));      // exactly 0 on all-masked rows (MASK_RAW c2 is exact)
            sum4[r] += p;
            sc[t][r] = p;
        }
    float sum = (sum4[0] + sum4[1]) + (sum4[2] + sum4[3]);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    return {ms, sum};
}

// ---- P, rounded to the operand type -----------------------------------------------------------------------------------------------------
// B operand of one 32-key P.V step: k-slot e of lane group g <-> key 32 kb + 4 g + e (tile 2 kb) | 32 kb + 16 + 4 g + (e - 4) (tile 2 kb + 1)
template <typename T>
__device__ __forceinline__ typename T::v8 attn_round_p(const f4& lo, const f4& hi) {
    typename T::v8 pf;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        pf[e] = T::from_f32(lo[e]);
        pf[4 + e] = T::from_f32(hi[e]);
    }
    return pf;
}
// ... and of the 16-key tail step
template <typename T>
__device__ __forceinline__ typename T::v4 attn_round_p_tail(const f4& s) {
    typename T::v4 pt;
#pragma unroll
    for (int e = 0; e < 4; ++e) pt[e] = T::from_f32(s[e]);
    return pt;
}

// ---- LDS image of one head, staged through registers (attention16_kernel, attention16_drop_kernel) ---------------------------------------
//   * K rows are 128 bytes, 16-byte slots XOR-swizzled with (row & 7): conflict-free ds_read_b128;
//   * V is transposed while staging, V^T[d][slot], so the A operand of the second product is ONE 16-byte LDS read per fragment;
//   * the per-key limits behind them.
template <int NT16>
struct AttnLds {
    static constexpr int SP = NT16 * 16;
    // V^T[d][slot], keys PERMUTED inside every group of 32 so that the eight contraction values a lane needs for one P.V step — keys
    // 32 kb + 4 g + (0..3) of score tile 2 kb and 32 kb + 16 + 4 g + (0..3) of tile 2 kb + 1 — are contiguous: key 16 t + 4 g' + r sits at slot
    // 32 (t >> 1) + 8 g' + 4 (t & 1) + r, and a fragment is ONE ds_read_b128 (round 6; before: two 8-byte pieces 32 bytes apart, read as a
    // ds_read2_b64 — 8 LDS cycles per wave-instruction instead of 4, MI355X_MICROARCH.md LDS table; the reads were a third of the kernel's LDS time).
    // Row stride: the slots an odd tile count leaves half-filled count, + 16 elements: rows 16 (mod 32) elements apart put the 16 rows of a
    // ds_read_b128 lane group on 16 distinct bank quads (208 -> 240: K + V^T + key limits = 58,176 B, two workgroups per CU as the registers allow).
    static constexpr int VT_LD = 32 * ((NT16 + 1) / 2) + 16;
    static constexpr int KP = (SP + 31) / 32;                // K passes of 256 threads: 32 rows per pass (the last may be partial: NT16 odd)
    static constexpr int VP = (SP / 4 + 31) / 32;            // V passes: 32 four-key groups per pass
    static constexpr int VT_OFF = SP * 128, KB_OFF = VT_OFF + 64 * VT_LD * 2, BYTES = KB_OFF + SP * 4;

    // byte offset of 16-byte chunk c of K row r
    static __device__ __forceinline__ int k_off(int r, int c) { return r * 128 + ((c ^ (r & 7)) << 4); }
    // where head dim d of the four keys 4 kg .. 4 kg + 3 sits in V^T
    template <class E>
    static __device__ __forceinline__ E* vt_at(E* sVt, int d, int kg) { return sVt + d * VT_LD + 32 * (kg >> 3) + 8 * (kg & 3) + 4 * ((kg >> 2) & 1); }

    // A operand of one P.V step out of V^T: head dim 16 dt + j, the lane group's eight contraction slots of 32-key step kb (V8; the
    // 16-key tail of an odd tile count reads the first four of step NT16 / 2 as a V4)
    template <class V, class E>
    static __device__ __forceinline__ V vt_frag(const E* sVt, int dt, int j, int g, int kb) {
        return *(const V*)(sVt + (dt * 16 + j) * VT_LD + kb * 32 + g * 8);
    }

    // stage chunk c of K row r (a thread of pass p: r = (tid >> 3) + 32 p, c = tid & 7)
    template <class V8>
    static __device__ __forceinline__ void stage_k_row(char* sK, int r, int c, const V8& k) {
        if (SP % 32 == 0 || r < SP) *(V8*)(sK + k_off(r, c)) = k;
    }
    // thread tid's share of V pass p: head dims 8 c .. 8 c + 7 of the four keys 4 kg .. 4 kg + 3 (c = tid & 7, kg = (tid >> 3) + 32 p, which the
    // caller has checked to be < SP / 4): eight 8-byte LDS writes.  Takes (tid, p), not (kg, c): hipcc optimises the helper before it inlines
    // it and needs to see where kg and c come from to form the addresses the written-out loop had
    template <typename T>
    static __device__ __forceinline__ void stage_v_group(typename T::elem* sVt, int tid, int p, const typename T::v8 (&v)[4]) {
        typedef typename T::v4 V4;
        const int c = tid & 7, kg = (tid >> 3) + 32 * p;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            V4 t;
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = v[r][e];
            *(V4*)vt_at(sVt, c * 8 + e, kg) = t;
        }
    }
};

// ---- context pack and store ---------------------------------------------------------------------------------------------------------------
// Rounds o * inv and writes the lane's share of context row `row` (element offset of the row's head slice from the wave-uniform `base`).
// A lane holds 4 consecutive head dims (8 B) of its query per 16-dim tile; lanes 16 apart (g, g+1) hold the neighbouring 8 B.
// `v_permlane16_swap` trades the odd lane group's piece of tile 2q for the even group's piece of tile 2q+1, so every lane owns 16
// contiguous bytes and a store instruction writes 16 rows x 64 contiguous bytes (two 16-byte stores per block instead of four 8-byte ones).
// Every lane takes part in the swaps; `store` = the lane's query is a real one.  `lane_group` returns g = lane >> 4 and is called inside
// the store predicate only (attention16_kernel recomputes it there, see its call).
// The offset is a 32-bit element offset from a wave-uniform base (the launchers check that an item's context is < 2^31 elements): as
// 64-bit per-lane addresses these were spilled in attention16_kernel, and every scratch reload is an `s_waitcnt vmcnt(0)`.
template <typename T, class G>
__device__ __forceinline__ void attn_store_ctx(typename T::elem* base, int row, G lane_group, const f4 (&o)[4], float inv, bool store) {
    typedef typename T::v4 V4;
    u2 pk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        V4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = T::from_f32(o[dt][r] * inv);
        pk[dt] = __builtin_bit_cast(u2, ov);
    }
#pragma unroll
    for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const auto sw = __builtin_amdgcn_permlane16_swap(pk[2 * q2][w], pk[2 * q2 + 1][w], false, false);
            pk[2 * q2][w] = sw[0];
            pk[2 * q2 + 1][w] = sw[1];
        }
    if (store) {
        const int g = lane_group();
        typename T::elem* op = base + (unsigned)(row + g * 4 + ((g & 1) ? 12 : 0));
#pragma unroll
        for (int q2 = 0; q2 < 2; ++q2)
            *(u4*)(op + q2 * 32) = (u4){pk[2 * q2][0], pk[2 * q2][1], pk[2 * q2 + 1][0], pk[2 * q2 + 1][1]};
    }
}
