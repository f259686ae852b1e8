// SASRec user encoder, ONE launch per direction (round 4).
// Replaces, for the production shape (d_model 64, sequences of <= 16 positions), the 15-launch forward and the ~34-launch backward
// of sasrec.hip — User_Encoder.forward (Code_Uncached/model/encoders.py:60-65) -> TransformerEncoder / TransformerBlock /
// MultiHeadedAttention / SelfAttention / PositionwiseFeedForward (Code_*/model/modules.py:6-96).  The whole encoder is ~2 MFLOP per
// sequence: as separate launches it cost 0.8 ms per step at ANY batch size (45 kernels of 5-25 us each: launch ramps and
// dependent-kernel boundaries), i.e. more than the in-batch CE of the Cached step.
//
// One 256-thread workgroup owns G = 48 / S consecutive sequences (R = G S <= 48 rows of 64 floats) from the position embedding to the
// last LayerNorm; the rows never leave LDS between operators.  Every product is [R, 64] x [64, 64]^T on `v_mfma_f32_16x16x4_f32`
// (exact fp32): wave w owns output columns 16 w ..+15 of all row tiles; the weight fragment comes straight from L2 (one 16-byte load
// per lane and 16 contraction steps — the contraction index of MFMA (t, e) is 16 t + 4 g + e, so both operands are 16-byte reads),
// the activation fragment is one conflict-free ds_read_b128 from a [48][68] LDS image.  The 64 -> 256 -> 64 FFN runs in four chunks
// of 64 hidden units whose second product accumulates in registers.  Attention (S x S per sequence and head), softmax, LayerNorm and
// the counter-based dropout (common.h: same sites and element indices as sasrec.hip) are plain per-thread / per-wave code on the LDS
// rows.  Every intermediate the backward needs is written to the same workspace slots sasrec.hip uses (coalesced 16-byte stores of
// whole LDS tiles), so either backward can follow either forward.
#include "common.h"

namespace {

constexpr int FE = 64;            // d_model
constexpr int FR = 48;            // rows per workgroup (3 MFMA row tiles): 4 sequences of 10 positions — one workgroup per CU at bs = 1024
constexpr int FLD = 68;           // LDS row stride (floats): 16 rows x 16 bytes of a ds_read_b128 lane group cover all 64 banks
constexpr int FNT = FR / 16;

struct FusedBlk {                  // per block: parameters and workspace slots (sasrec.hip: BlockBufs)
    const float *wq, *wk, *wv, *wfc, *ln1g, *ln1b, *w1, *b1, *w2, *b2, *ln2g, *ln2b;
    float *Q, *K, *V, *P, *C, *Zattn, *X1, *Hf, *Zffn, *X2;
};
struct FusedFwdArgs {
    const float* x; const float* log_mask; const float* pos; const float* ln0g; const float* ln0b;
    float* Z0; float* X0; float* y;
    FusedBlk blk[8];
    int64_t B; int32_t S, H, blocks, G;       // G sequences per workgroup
    uint64_t seed; uint32_t thr24; float inv_keep;
    long long* stamps;                        // development aid: cycle stamps of workgroup 0 at the stage boundaries (null in the product)
};

__device__ __forceinline__ float dropf(const FusedFwdArgs& a, uint32_t site, uint64_t idx) {
    return a.thr24 ? drop_scale(a.seed, site, idx, a.thr24, a.inv_keep) : 1.0f;
}

// acc[rt] (+)= X[16 rt .. +15, 0..63] . W[n0 .. n0+15, 0..63]^T   (X: LDS image, W: global, row stride ldw floats).  The weight
// fragment (four 16-byte loads per lane, L2) is requested by load_w() ahead of time — a product that waits for its own loads spends
// ~1,000 of its ~2,900 cycles there (stage timeline) — and consumed by tile_product_w().
struct WFrag { f4 v[4]; };
__device__ __forceinline__ WFrag load_w(const float* __restrict__ W, int ldw, int n0, int lane) {
    const int i = lane & 15, g = lane >> 4;
    WFrag w;
#pragma unroll
    for (int t = 0; t < 4; ++t) w.v[t] = *(const f4*)(W + (int64_t)(n0 + i) * ldw + 16 * t + 4 * g);
    return w;
}
__device__ __forceinline__ void tile_product_w(const float* __restrict__ X, const WFrag& w, int lane, f4 (&acc)[FNT]) {
    const int i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        f4 xa[FNT];
#pragma unroll
        for (int rt = 0; rt < FNT; ++rt) xa[rt] = *(const f4*)(X + (16 * rt + i) * FLD + 16 * t + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e)          // consecutive MFMAs on DIFFERENT accumulators (40-cycle dependent latency, 32-cycle issue)
#pragma unroll
            for (int rt = 0; rt < FNT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt][e], w.v[t][e], acc[rt], 0, 0, 0);
    }
}
__device__ __forceinline__ void tile_product(const float* __restrict__ X, const float* __restrict__ W, int ldw, int n0, int lane,
                                             f4 (&acc)[FNT]) {
    tile_product_w(X, load_w(W, ldw, n0, lane), lane, acc);
}
__device__ __forceinline__ void zero_acc(f4 (&acc)[FNT]) {
#pragma unroll
    for (int rt = 0; rt < FNT; ++rt) acc[rt] = (f4){0.f, 0.f, 0.f, 0.f};
}
// accumulator element r of lane (j, g) in row tile rt is (row 16 rt + 4 g + r, column n0 + j)
template <typename F>
__device__ __forceinline__ void for_acc(const f4 (&acc)[FNT], int n0, int lane, F&& f) {
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int rt = 0; rt < FNT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) f(16 * rt + 4 * g + r, n0 + j, acc[rt][r]);
}
// LDS tile rows [0, nrows) x 64 -> global rows row0 .. (row stride ld floats, column offset c0), 16 bytes per thread and piece
__device__ __forceinline__ void store_tile(const float* buf, float* gp, int64_t row0, int ld, int c0, int nrows, int tid) {
    for (int p = tid; p < nrows * 16; p += 256) {
        const int r = p >> 4, c = (p & 15) * 4;
        *(f4*)(gp + (row0 + r) * ld + c0 + c) = *(const f4*)(buf + r * FLD + c);
    }
}
// y = LN(z) * g + b over the 64 columns of rows [0, nrows): a wave takes FOUR rows at a time (16 lanes per row, 4 columns per lane,
// two 4-step xor reductions) — one row per wave and pass was a serial chain of ~1,000 cycles per row (stage timeline: 21k cycles
// per LayerNorm of 80 rows)
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ void ln_rows(const float* z, float* y, const float* __restrict__ g, const float* __restrict__ b,
                                        int nrows, int wave, int lane) {
    const int c = (lane & 15) * 4;
    const f4 gg = *(const f4*)(g + c), bb = *(const f4*)(b + c);
    for (int r = wave * 4 + (lane >> 4); r < nrows; r += 16) {           // (rows past nrows: the whole 16-lane group skips)
        const f4 v = *(const f4*)(z + r * FLD + c);
        const float mean = sum16(v[0] + v[1] + v[2] + v[3]) * (1.0f / 64.0f);
        const f4 d = v - mean;
        const float rstd = rsqrtf(sum16(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]) * (1.0f / 64.0f) + 1e-6f);
        *(f4*)(y + r * FLD + c) = d * rstd * gg + bb;
    }
}

template <int DH>
__global__ __launch_bounds__(256) void sasrec_fused_fwd_kernel(FusedFwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* bX = sm;                      // block input / output
    float* bA = bX + FR * FLD;           // Q -> C -> Hf chunk
    float* bB = bA + FR * FLD;           // K -> Zattn -> Zffn
    float* bC = bB + FR * FLD;           // V -> X1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, H = a.H;
    constexpr int dh = DH;
    const int64_t b0 = (int64_t)blockIdx.x * a.G;
    const int nseq = (int)((a.B - b0) < a.G ? (a.B - b0) : a.G);
    const int R = nseq * S;
    const int64_t row0 = b0 * S;
    const int n0 = 16 * wave;
    int nst = 0;
    auto stamp = [&]() { if (a.stamps && blockIdx.x == 0 && tid == 0) a.stamps[nst++] = __builtin_readcyclecounter(); };
    stamp();
    // rows R .. FR-1 of every buffer are read by the MFMAs of the last row tile: keep them finite
    for (int p = tid; p < 4 * (FR - R) * FLD; p += 256) {
        const int bf = p / ((FR - R) * FLD), o = p - bf * ((FR - R) * FLD);
        sm[bf * FR * FLD + R * FLD + o] = 0.f;
    }
    // ---- X0 = drop(LN(x + pos)) ----
    for (int p = tid; p < R * 16; p += 256) {
        const int r = p >> 4, c = (p & 15) * 4;
        const f4 xv = *(const f4*)(a.x + (row0 + r) * FE + c), pv = *(const f4*)(a.pos + (r % S) * FE + c);
        *(f4*)(bB + r * FLD + c) = xv + pv;
    }
    __syncthreads();
    store_tile(bB, a.Z0, row0, FE, 0, R, tid);
    ln_rows(bB, bX, a.ln0g, a.ln0b, R, wave, lane);
    __syncthreads();
    if (a.thr24) {
        for (int p = tid; p < R * 64; p += 256) {
            const int r = p >> 6, c = p & 63;
            bX[r * FLD + c] *= dropf(a, 0, (uint64_t)((row0 + r) * FE + c));
        }
        __syncthreads();
    }
    store_tile(bX, a.X0, row0, FE, 0, R, tid);
    stamp();       // 1: embedding LN done
    const float temp = sqrtf((float)dh);
#pragma unroll 1
    for (int l = 0; l < a.blocks; ++l) {
        const FusedBlk& k = a.blk[l];
        // ---- Q, K, V ----
        {
            const WFrag fq = load_w(k.wq, FE, n0, lane), fk = load_w(k.wk, FE, n0, lane), fv = load_w(k.wv, FE, n0, lane);
            f4 acc[FNT];
            zero_acc(acc); tile_product_w(bX, fq, lane, acc);
            for_acc(acc, n0, lane, [&](int r, int c, float v) { bA[r * FLD + c] = v; });
            zero_acc(acc); tile_product_w(bX, fk, lane, acc);
            for_acc(acc, n0, lane, [&](int r, int c, float v) { bB[r * FLD + c] = v; });
            zero_acc(acc); tile_product_w(bX, fv, lane, acc);
            for_acc(acc, n0, lane, [&](int r, int c, float v) { bC[r * FLD + c] = v; });
        }
        __syncthreads();
        stamp();   // QKV products
        store_tile(bA, k.Q, row0, FE, 0, R, tid);
        store_tile(bB, k.K, row0, FE, 0, R, tid);
        store_tile(bC, k.V, row0, FE, 0, R, tid);
        __syncthreads();                                  // (Q is overwritten in place by the attention threads)
        // ---- attention: ONE THREAD per (sequence, head, query) — scores, softmax and P.V in registers (S <= 16, dh <= 64).  The thread
        //      reads its own Q row slice and overwrites exactly that slice of bA with C, so no barrier separates the three steps.
        //      (first version: scores / softmax / P.V as three barrier-separated loops over LDS with index divisions — 26k + 6k + 21k
        //      cycles per block in the stage timeline)
        if (tid < nseq * H * S) {
            const int sh = tid / S, q = tid - sh * S;
            const int sq = sh / H, h = sh - sq * H;
            float* qrow = bA + (sq * S + q) * FLD + h * dh;
            f4 qa[DH / 4];
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) qa[e] = *(const f4*)(qrow + 4 * e);
            float sc[16];
            float mx = -INFINITY;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                if (kk < S) {
                    const float* kr = bB + (sq * S + kk) * FLD + h * dh;
                    f4 kb[DH / 4];
#pragma unroll
                    for (int e = 0; e < DH / 4; ++e) kb[e] = *(const f4*)(kr + 4 * e);
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < DH / 4; ++e) { d += qa[e][0] * kb[e][0]; d += qa[e][1] * kb[e][1]; d += qa[e][2] * kb[e][2]; d += qa[e][3] * kb[e][3]; }
                    const float m = (kk <= q && a.log_mask[(b0 + sq) * S + kk] != 0.f) ? 0.f : -1e9f;
                    sc[kk] = d / temp + m;
                    mx = fmaxf(mx, sc[kk]);
                }
            }
            float sum = 0.f;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                if (kk < S) { sc[kk] = expf(sc[kk] - mx); sum += sc[kk]; }
            const int64_t gp = ((b0 * H + sh) * S + q) * S;            // ((b H + h) S + q) S with b = b0 + sq
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                if (kk < S) {
                    const float pr = sc[kk] / sum;
                    k.P[gp + kk] = pr;                                  // probabilities BEFORE dropout are kept for the backward
                    sc[kk] = pr * dropf(a, 1 + 3 * l, (uint64_t)(gp + kk));
                }
            f4 oc[DH / 4];
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) oc[e] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                if (kk < S) {
                    const float* vr = bC + (sq * S + kk) * FLD + h * dh;
#pragma unroll
                    for (int e = 0; e < DH / 4; ++e) oc[e] += sc[kk] * *(const f4*)(vr + 4 * e);
                }
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) *(f4*)(qrow + 4 * e) = oc[e];
        }
        __syncthreads();
        stamp();   // attention
        store_tile(bA, k.C, row0, FE, 0, R, tid);
        // ---- Zattn = X + drop(C Wfc^T) -> bB (K is dead);  X1 = LN(Zattn) -> bC (V is dead) ----
        {
            f4 acc[FNT];
            zero_acc(acc); tile_product(bA, k.wfc, FE, n0, lane, acc);
            for_acc(acc, n0, lane, [&](int r, int c, float v) {
                bB[r * FLD + c] = bX[r * FLD + c] + v * dropf(a, 2 + 3 * l, (uint64_t)((row0 + r) * FE + c));
            });
        }
        __syncthreads();
        stamp();   // fc product
        store_tile(bB, k.Zattn, row0, FE, 0, R, tid);
        ln_rows(bB, bC, k.ln1g, k.ln1b, R, wave, lane);
        __syncthreads();
        stamp();   // LN1
        store_tile(bC, k.X1, row0, FE, 0, R, tid);
        // ---- FFN in four chunks of 64 hidden units: Hf_c = relu(X1 W1_c^T + b1_c) -> bA; out += Hf_c W2[:, c]^T ----
        f4 out[FNT];
        zero_acc(out);
        WFrag f1 = load_w(k.w1, FE, n0, lane);
#pragma unroll 1
        for (int c4 = 0; c4 < 4; ++c4) {
            const WFrag f2 = load_w(k.w2 + c4 * 64, 4 * FE, n0, lane);          // in flight during the first product
            f4 acc[FNT];
            zero_acc(acc); tile_product_w(bC, f1, lane, acc);
            if (c4 < 3) f1 = load_w(k.w1 + (int64_t)(c4 + 1) * 64 * FE, FE, n0, lane);       // the next chunk's, during the second product
            const float bias1 = k.b1[c4 * 64 + n0 + (lane & 15)];      // the lane's column
            if (c4) __syncthreads();                 // the previous chunk's readers are done with bA
            for_acc(acc, n0, lane, [&](int r, int c, float v) { bA[r * FLD + c] = fmaxf(v + bias1, 0.f); });
            __syncthreads();
            store_tile(bA, k.Hf, row0, 4 * FE, c4 * 64, R, tid);
            tile_product_w(bA, f2, lane, out);
        }
        // ---- Zffn = X1 + drop(out + b2) -> bB (Zattn is dead);  X2 = LN(Zffn) -> bX ----
        const float bias2 = k.b2[n0 + (lane & 15)];
        for_acc(out, n0, lane, [&](int r, int c, float v) {
            bB[r * FLD + c] = bC[r * FLD + c] + (v + bias2) * dropf(a, 3 + 3 * l, (uint64_t)((row0 + r) * FE + c));
        });
        __syncthreads();
        stamp();   // FFN
        store_tile(bB, k.Zffn, row0, FE, 0, R, tid);
        ln_rows(bB, bX, k.ln2g, k.ln2b, R, wave, lane);
        __syncthreads();
        stamp();   // LN2
        store_tile(bX, l == a.blocks - 1 ? a.y : k.X2, row0, FE, 0, R, tid);
    }
}


// =====================================================================================================================
// backward: the same row partition; parameter gradients leave as one slab of partial sums per workgroup (reduced by
// sasrec_reduce_kernel in a fixed order: bit-reproducible, no atomics)
// =====================================================================================================================
struct FusedBwdArgs {
    const float* dy; const float* log_mask; float* dx;
    const float* Z0; const float* X0; const float* ln0g;
    FusedBlk blk[8];
    float* slab; int64_t slab_stride;
    int64_t B; int32_t S, H, blocks, G;
    uint64_t seed; uint32_t thr24; float inv_keep;
};
// slab layout (floats): [0, 1024) dpos | 1024 dln0.g | 1088 dln0.b | 1152 + l * SLAB_BLK: one block's gradients
constexpr int SLAB_POS = 0, SLAB_LN0G = 1024, SLAB_LN0B = 1088, SLAB_BLK0 = 1152;
constexpr int SB_WQ = 0, SB_WK = 4096, SB_WV = 8192, SB_WFC = 12288, SB_LN1G = 16384, SB_LN1B = 16448, SB_W1 = 16512, SB_B1 = 32896,
              SB_W2 = 33152, SB_B2 = 49536, SB_LN2G = 49600, SB_LN2B = 49664, SLAB_BLK = 49728;

__device__ __forceinline__ float dropb(const FusedBwdArgs& a, uint32_t site, uint64_t idx) {
    return a.thr24 ? drop_scale(a.seed, site, idx, a.thr24, a.inv_keep) : 1.0f;
}
// weight fragment for a product that contracts over the ROWS of W:  B[k][j] = W[k * ld + n0 + j]  (dX = dY . W)
__device__ __forceinline__ WFrag load_wT(const float* __restrict__ W, int ld, int n0, int lane) {
    const int j = lane & 15, g = lane >> 4;
    WFrag w;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) w.v[t][e] = W[(int64_t)(16 * t + 4 * g + e) * ld + n0 + j];
    return w;
}
// global rows -> LDS tile (rows [0, nrows) x 64; pad rows are never written by anyone and stay zero)
__device__ __forceinline__ void load_tile(float* buf, const float* gp, int64_t row0, int ld, int c0, int nrows, int tid) {
    for (int p = tid; p < nrows * 16; p += 256) {
        const int r = p >> 4, c = (p & 15) * 4;
        *(f4*)(buf + r * FLD + c) = *(const f4*)(gp + (row0 + r) * ld + c0 + c);
    }
}
// dW[i0 + .., 0..63] = A[:, i0 + ..]^T . B   (contraction over the FR rows of two LDS tiles; A's pad rows are zero).  Wave w owns
// output rows 16 w ..+15 and all four column tiles; results go to dst[(row) * ldd + col].
__device__ __forceinline__ void tile_dw(const float* A, const float* Bm, float* dst, int ldd, int wave, int lane) {
    const int i = lane & 15, g = lane >> 4, i0 = 16 * wave;
    f4 acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) acc[ct] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < FNT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kr = (16 * t + 4 * g + e) * FLD;
            const float av = A[kr + i0 + i];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bm[kr + 16 * ct + i], acc[ct], 0, 0, 0);
        }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(int64_t)(i0 + 4 * g + r) * ldd + 16 * ct + i] = acc[ct][r];
}
// column sums over the rows of an LDS tile -> dst[0..63]
__device__ __forceinline__ void tile_colsum(const float* buf, float* dst, int nrows, int tid) {
    if (tid < 64) {
        float s = 0.f;
        for (int r = 0; r < nrows; ++r) s += buf[r * FLD + tid];
        dst[tid] = s;
    }
}
// LayerNorm backward over rows [0, nrows) of z (pre-norm input) with upstream dy (optionally times the embedding dropout factors):
// dz -> out;  partial dgamma / dbeta of the workgroup -> dg[0..63], db[0..63] (through sRed[2][4][64])
__device__ __forceinline__ void ln_bwd_rows(const FusedBwdArgs& a, const float* z, const float* dy, const float* __restrict__ g,
                                            float* out, float* dgo, float* dbo, float* sRed, int nrows, int64_t row0, bool drop0,
                                            int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const int c = (lane & 15) * 4;
    const f4 gg = *(const f4*)(g + c);
    f4 dg = {0.f, 0.f, 0.f, 0.f}, db = {0.f, 0.f, 0.f, 0.f};
    for (int r = wave * 4 + (lane >> 4); r < nrows; r += 16) {
        const f4 v = *(const f4*)(z + r * FLD + c);
        f4 d = *(const f4*)(dy + r * FLD + c);
        if (drop0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] *= dropb(a, 0, (uint64_t)((row0 + r) * FE + c + e));
        }
        const float mean = sum16(v[0] + v[1] + v[2] + v[3]) * (1.0f / 64.0f);
        const f4 vc = v - mean;
        const float rstd = rsqrtf(sum16(vc[0] * vc[0] + vc[1] * vc[1] + vc[2] * vc[2] + vc[3] * vc[3]) * (1.0f / 64.0f) + 1e-6f);
        const f4 xh = vc * rstd;
        dg += d * xh;
        db += d;
        const f4 dgm = d * gg;
        const float s1 = sum16(dgm[0] + dgm[1] + dgm[2] + dgm[3]) * (1.0f / 64.0f);
        const float s2 = sum16(dgm[0] * xh[0] + dgm[1] * xh[1] + dgm[2] * xh[2] + dgm[3] * xh[3]) * (1.0f / 64.0f);
        *(f4*)(out + r * FLD + c) = rstd * (dgm - s1 - xh * s2);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        dg[e] += __shfl_xor(dg[e], 16, 64); dg[e] += __shfl_xor(dg[e], 32, 64);
        db[e] += __shfl_xor(db[e], 16, 64); db[e] += __shfl_xor(db[e], 32, 64);
    }
    if (lane < 16) {
        *(f4*)(sRed + wave * 64 + c) = dg;
        *(f4*)(sRed + 256 + wave * 64 + c) = db;
    }
    __syncthreads();
    if (tid < 64) {
        dgo[tid] = (sRed[tid] + sRed[64 + tid]) + (sRed[128 + tid] + sRed[192 + tid]);
        dbo[tid] = (sRed[256 + tid] + sRed[320 + tid]) + (sRed[384 + tid] + sRed[448 + tid]);
    }
}

template <int DH>
__global__ __launch_bounds__(256) void sasrec_fused_bwd_kernel(FusedBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int TB = FR * FLD;
    float* bG = sm;              // incoming gradient of the block output / outgoing gradient of its input
    float* bZ = bG + TB;         // forward tensor of the LayerNorm being differentiated
    float* bA = bZ + TB;         // dZ (LayerNorm backward output)
    float* bF = bA + TB;         // dZ times the dropout factors of the branch
    float* bX = bF + TB;         // X1, later the block input
    float* bH = bX + TB;         // Hf chunk / C / Q
    float* bD = bH + TB;         // dHf chunk / dC
    float* bK = bD + TB;         // K -> dK
    float* bV = bK + TB;         // V -> dV
    float* bQ = bF;              // dQ (the branch gradient is dead by then)
    float* sS = bV + TB;         // dS   [attention threads <= 192][16]
    float* sM = sS + 192 * 16;   // P * dropout factors
    float* sRed = sM + 192 * 16; // [2][4][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, H = a.H;
    constexpr int dh = DH;
    const int64_t b0 = (int64_t)blockIdx.x * a.G;
    const int nseq = (int)((a.B - b0) < a.G ? (a.B - b0) : a.G);
    const int R = nseq * S;
    const int64_t row0 = b0 * S;
    const int n0 = 16 * wave;
    float* slab = a.slab + (int64_t)blockIdx.x * a.slab_stride;
    const float temp = sqrtf((float)dh);
    const bool drop = a.thr24 != 0;
    // pad rows of every tile: zero, and never written afterwards (they are the tail of the K = rows contractions)
    for (int p = tid; p < 9 * TB; p += 256) sm[p] = 0.f;
    __syncthreads();
    load_tile(bG, a.dy, row0, FE, 0, R, tid);
    // guarded accumulator store: rows < R only
    auto put = [&](float* buf, const f4 (&acc)[FNT], auto&& f) {
        const int j = lane & 15, g = lane >> 4;
#pragma unroll
        for (int rt = 0; rt < FNT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * rt + 4 * g + r;
                if (row < R) buf[row * FLD + n0 + j] = f(row, n0 + j, acc[rt][r]);
            }
    };
#pragma unroll 1
    for (int l = a.blocks - 1; l >= 0; --l) {
        const FusedBlk& k = a.blk[l];
        float* sb = slab + SLAB_BLK0 + l * SLAB_BLK;
        // ---- X2 = LN(Zffn): dZffn -> bA ----
        load_tile(bZ, k.Zffn, row0, FE, 0, R, tid);
        load_tile(bX, k.X1, row0, FE, 0, R, tid);
        __syncthreads();
        ln_bwd_rows(a, bZ, bG, k.ln2g, bA, sb + SB_LN2G, sb + SB_LN2B, sRed, R, row0, false, tid);
        __syncthreads();
        // the FFN branch sees dZffn times the forward keep factors (Zffn = X1 + drop(Hf W2^T + b2))
        const float* gF = bA;
        if (drop) {
            for (int p = tid; p < R * 64; p += 256) {
                const int r = p >> 6, c = p & 63;
                bF[r * FLD + c] = bA[r * FLD + c] * dropb(a, 3 + 3 * l, (uint64_t)((row0 + r) * FE + c));
            }
            gF = bF;
            __syncthreads();
        }
        tile_colsum(gF, sb + SB_B2, R, tid);
        f4 dx1[FNT];
        zero_acc(dx1);
#pragma unroll 1
        for (int c4 = 0; c4 < 4; ++c4) {
            const WFrag f2 = load_wT(k.w2 + c4 * 64, 4 * FE, n0, lane);
            const WFrag f1 = load_wT(k.w1 + (int64_t)c4 * 64 * FE, FE, n0, lane);
            load_tile(bH, k.Hf, row0, 4 * FE, c4 * 64, R, tid);
            f4 acc[FNT];
            zero_acc(acc); tile_product_w(gF, f2, lane, acc);                  // gF . W2[:, chunk]
            __syncthreads();                                                    // Hf chunk landed; bD free (previous chunk's readers done)
            put(bD, acc, [&](int r, int c, float v) { return bH[r * FLD + c] > 0.f ? v : 0.f; });      // dHf = (.) * [Hf > 0]
            __syncthreads();
            tile_dw(gF, bH, sb + SB_W2 + c4 * 64, 4 * FE, wave, lane);         // dW2[:, chunk] = gF^T Hf
            tile_dw(bD, bX, sb + SB_W1 + c4 * 64 * FE, FE, wave, lane);        // dW1[chunk, :] = dHf^T X1
            tile_colsum(bD, sb + SB_B1 + c4 * 64, R, tid);
            tile_product_w(bD, f1, lane, dx1);                                  // dX1 += dHf . W1[chunk, :]
            __syncthreads();                                                    // bH / bD are rewritten by the next chunk
        }
        put(bG, dx1, [&](int r, int c, float v) { return bA[r * FLD + c] + v; });      // dX1 = dZffn + sum
        // ---- X1 = LN(Zattn): dZattn -> bA ----
        load_tile(bZ, k.Zattn, row0, FE, 0, R, tid);
        load_tile(bH, k.C, row0, FE, 0, R, tid);
        __syncthreads();
        ln_bwd_rows(a, bZ, bG, k.ln1g, bA, sb + SB_LN1G, sb + SB_LN1B, sRed, R, row0, false, tid);
        __syncthreads();
        const float* gA = bA;
        if (drop) {
            for (int p = tid; p < R * 64; p += 256) {
                const int r = p >> 6, c = p & 63;
                bF[r * FLD + c] = bA[r * FLD + c] * dropb(a, 2 + 3 * l, (uint64_t)((row0 + r) * FE + c));
            }
            gA = bF;
            __syncthreads();
        }
        // ---- Zattn = xin + drop(C Wfc^T): dC = gA . Wfc -> bD;  dWfc = gA^T C ----
        {
            const WFrag ff = load_wT(k.wfc, FE, n0, lane);
            f4 acc[FNT];
            zero_acc(acc); tile_product_w(gA, ff, lane, acc);
            put(bD, acc, [&](int, int, float v) { return v; });
            tile_dw(gA, bH, sb + SB_WFC, FE, wave, lane);
        }
        __syncthreads();
        load_tile(bH, k.Q, row0, FE, 0, R, tid);
        load_tile(bK, k.K, row0, FE, 0, R, tid);
        load_tile(bV, k.V, row0, FE, 0, R, tid);
        const float* xin = l == 0 ? a.X0 : a.blk[l - 1].X2;     // the block input: drop(LN(Z0)) or the previous block's output
        __syncthreads();
        // ---- attention backward, phase 1: one thread per (sequence, head, query) — dP, dS, dQ ----
        if (tid < nseq * H * S) {
            const int sh = tid / S, q = tid - sh * S;
            const int sq = sh / H, h = sh - sq * H;
            const int64_t gp = ((b0 * H + sh) * S + q) * S;
            f4 dc[DH / 4];
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) dc[e] = *(const f4*)(bD + (sq * S + q) * FLD + h * dh + 4 * e);
            float pr[16], dP[16];
            float dot = 0.f;
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                if (kk < S) {
                    const float* vr = bV + (sq * S + kk) * FLD + h * dh;
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < DH / 4; ++e) {
                        const f4 vv = *(const f4*)(vr + 4 * e);
                        d += dc[e][0] * vv[0]; d += dc[e][1] * vv[1]; d += dc[e][2] * vv[2]; d += dc[e][3] * vv[3];
                    }
                    const float mk = dropb(a, 1 + 3 * l, (uint64_t)(gp + kk));
                    pr[kk] = k.P[gp + kk];
                    dP[kk] = d * mk;
                    sM[tid * 16 + kk] = pr[kk] * mk;
                    dot += pr[kk] * dP[kk];
                }
            f4 dq[DH / 4];
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) dq[e] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk)
                if (kk < S) {
                    const float ds = pr[kk] * (dP[kk] - dot) / temp;
                    sS[tid * 16 + kk] = ds;
                    const float* kr = bK + (sq * S + kk) * FLD + h * dh;
#pragma unroll
                    for (int e = 0; e < DH / 4; ++e) dq[e] += ds * *(const f4*)(kr + 4 * e);
                }
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) *(f4*)(bQ + (sq * S + q) * FLD + h * dh + 4 * e) = dq[e];
        }
        __syncthreads();
        // ---- phase 2: one thread per (sequence, head, key) — dK = dS^T Q, dV = (P * mask)^T dC, in place over K / V ----
        if (tid < nseq * H * S) {
            const int sh = tid / S, kk = tid - sh * S;
            const int sq = sh / H, h = sh - sq * H;
            f4 dk[DH / 4], dv[DH / 4];
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) { dk[e] = (f4){0.f, 0.f, 0.f, 0.f}; dv[e] = (f4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int q = 0; q < 16; ++q)
                if (q < S) {
                    const float ds = sS[(sh * S + q) * 16 + kk], pm = sM[(sh * S + q) * 16 + kk];
                    const float* qr = bH + (sq * S + q) * FLD + h * dh;
                    const float* cr = bD + (sq * S + q) * FLD + h * dh;
#pragma unroll
                    for (int e = 0; e < DH / 4; ++e) { dk[e] += ds * *(const f4*)(qr + 4 * e); dv[e] += pm * *(const f4*)(cr + 4 * e); }
                }
#pragma unroll
            for (int e = 0; e < DH / 4; ++e) {
                *(f4*)(bK + (sq * S + kk) * FLD + h * dh + 4 * e) = dk[e];
                *(f4*)(bV + (sq * S + kk) * FLD + h * dh + 4 * e) = dv[e];
            }
        }
        load_tile(bX, xin, row0, FE, 0, R, tid);
        __syncthreads();
        tile_dw(bQ, bX, sb + SB_WQ, FE, wave, lane);
        tile_dw(bK, bX, sb + SB_WK, FE, wave, lane);
        tile_dw(bV, bX, sb + SB_WV, FE, wave, lane);
        {
            const WFrag fq = load_wT(k.wq, FE, n0, lane), fk = load_wT(k.wk, FE, n0, lane), fv = load_wT(k.wv, FE, n0, lane);
            f4 acc[FNT];
            zero_acc(acc);
            tile_product_w(bQ, fq, lane, acc);
            tile_product_w(bK, fk, lane, acc);
            tile_product_w(bV, fv, lane, acc);
            put(bG, acc, [&](int r, int c, float v) { return bA[r * FLD + c] + v; });     // dxin = dZattn + dQ Wq + dK Wk + dV Wv
        }
        __syncthreads();
    }
    // ---- X0 = drop(LN(Z0)), Z0 = x + pos: dx, dln0, dpos ----
    load_tile(bZ, a.Z0, row0, FE, 0, R, tid);
    __syncthreads();
    ln_bwd_rows(a, bZ, bG, a.ln0g, bA, slab + SLAB_LN0G, slab + SLAB_LN0B, sRed, R, row0, drop, tid);
    __syncthreads();
    store_tile(bA, a.dx, row0, FE, 0, R, tid);
    for (int p = tid; p < S * 64; p += 256) {
        const int sp = p >> 6, c = p & 63;
        float s = 0.f;
        for (int sq = 0; sq < nseq; ++sq) s += bA[(sq * S + sp) * FLD + c];
        slab[SLAB_POS + p] = s;
    }
}

// grads[i][e] += sum over workgroups of slab[wg][off_i + e]   (ascending workgroup order: reproducible)
struct ReduceTab { float* g[100]; int32_t off[100]; int32_t cnt[100]; int32_t n; };
__global__ __launch_bounds__(256) void sasrec_reduce_kernel(const float* __restrict__ slab, int64_t stride, int nwg, ReduceTab t) {
    const int i = blockIdx.y;
    if (i >= t.n) return;
    // one element per thread, eight independent partial sums (a fixed tree: reproducible); the 16-element version with 16 workgroups
    // per tensor took 84 us at bs = 1024 (256 slabs x 100 K floats = 103 MB at 1.2 TB/s)
    for (int e = blockIdx.x * 256 + threadIdx.x; e < t.cnt[i]; e += gridDim.x * 256) {
        const float* p = slab + t.off[i] + e;
        float sacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int w = 0;
        for (; w + 8 <= nwg; w += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) sacc[u] += p[(int64_t)(w + u) * stride];
        }
        for (; w < nwg; ++w) sacc[0] += p[(int64_t)w * stride];
        t.g[i][e] += ((sacc[0] + sacc[1]) + (sacc[2] + sacc[3])) + ((sacc[4] + sacc[5]) + (sacc[6] + sacc[7]));
    }
}

}  // namespace

// The fused path covers the production configuration; anything else stays on the per-operator launches of sasrec.hip.
static int g_sasrec_fused = 1;
static constexpr long long* g_sasrec_stamps = nullptr;      // (the stage-timeline switch of tools/sasrec_stamps.py was retired in round 5)
IISAN_DEV_KNOB(sasrec_fused, g_sasrec_fused);
bool sasrec_fused_shape_ok(const iisan_sasrec_cfg* cfg) {       // (the workspace is sized by this alone: the knob only picks kernels)
    return cfg->emb == FE && cfg->seq >= 1 && cfg->seq <= 16 && cfg->heads >= 1 && FE % cfg->heads == 0 &&
           (cfg->heads == 1 || cfg->heads == 2 || cfg->heads == 4) && (FR / cfg->seq) * cfg->heads * cfg->seq <= 192 && cfg->blocks >= 1 && cfg->blocks <= 8;
}
bool sasrec_fused_ok(const iisan_sasrec_cfg* cfg) { return g_sasrec_fused && sasrec_fused_shape_ok(cfg); }

int64_t sasrec_fused_slab_floats(const iisan_sasrec_cfg* cfg, int64_t B) {
    return ceil_div(B, FR / cfg->seq) * (int64_t)(SLAB_BLK0 + cfg->blocks * SLAB_BLK);
}

static int64_t g_cnt_sasrec_fused = 0;       // one-launch SASRec forward passes (route counter, common.h)
IISAN_DEV_COUNTER(sasrec_fused_fwd, g_cnt_sasrec_fused);

int launch_sasrec_fused_fwd(const iisan_sasrec_cfg* cfg, const float* x, const float* log_mask, int64_t B, const void* const* params,
                            float* y, const SasFusedPtrs& w, hipStream_t s) {
    ++g_cnt_sasrec_fused;
    FusedFwdArgs a{};
    auto W = [&](int i) { return (const float*)params[i]; };
    a.x = x; a.log_mask = log_mask; a.pos = W(0); a.ln0g = W(1); a.ln0b = W(2);
    a.Z0 = w.Z0; a.X0 = w.X0; a.y = y;
    for (int l = 0; l < cfg->blocks; ++l) {
        FusedBlk& k = a.blk[l];
        const int p = 3 + 12 * l;
        k.wq = W(p); k.wk = W(p + 1); k.wv = W(p + 2); k.wfc = W(p + 3); k.ln1g = W(p + 4); k.ln1b = W(p + 5);
        k.w1 = W(p + 6); k.b1 = W(p + 7); k.w2 = W(p + 8); k.b2 = W(p + 9); k.ln2g = W(p + 10); k.ln2b = W(p + 11);
        k.Q = w.Q[l]; k.K = w.K[l]; k.V = w.V[l]; k.P = w.P[l]; k.C = w.C[l]; k.Zattn = w.Zattn[l]; k.X1 = w.X1[l];
        k.Hf = w.Hf[l]; k.Zffn = w.Zffn[l]; k.X2 = w.X2[l];
    }
    a.B = B; a.S = cfg->seq; a.H = cfg->heads; a.blocks = cfg->blocks; a.G = FR / cfg->seq;
    const DropCfg d = make_drop(cfg->seed, 0, cfg->dropout);
    a.seed = d.seed; a.thr24 = d.thr24; a.inv_keep = d.inv_keep;
    a.stamps = g_sasrec_stamps;
    const size_t lds = (size_t)(4 * FR * FLD) * sizeof(float);
    const dim3 grid((unsigned)ceil_div(B, a.G));
    switch (FE / cfg->heads) {
        case 64: hipLaunchKernelGGL(sasrec_fused_fwd_kernel<64>, grid, dim3(256), lds, s, a); break;
        case 32: hipLaunchKernelGGL(sasrec_fused_fwd_kernel<32>, grid, dim3(256), lds, s, a); break;
        case 16: hipLaunchKernelGGL(sasrec_fused_fwd_kernel<16>, grid, dim3(256), lds, s, a); break;
        default: iisan_set_error("sasrec_fused: head width %d not instantiated", FE / cfg->heads); return IISAN_EBADSHAPE;
    }
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

int launch_sasrec_fused_bwd(const iisan_sasrec_cfg* cfg, const float* log_mask, int64_t B, const void* const* params, const float* dy,
                            float* dx, void* const* grads, const SasFusedPtrs& w, float* slab, hipStream_t s) {
    FusedBwdArgs a{};
    auto W = [&](int i) { return (const float*)params[i]; };
    a.dy = dy; a.log_mask = log_mask; a.dx = dx; a.Z0 = w.Z0; a.X0 = w.X0; a.ln0g = W(1);
    ReduceTab tab{};
    auto add = [&](int pi, int off, int cnt) { tab.g[tab.n] = (float*)grads[pi]; tab.off[tab.n] = off; tab.cnt[tab.n] = cnt; ++tab.n; };
    add(0, SLAB_POS, cfg->seq * FE); add(1, SLAB_LN0G, FE); add(2, SLAB_LN0B, FE);
    for (int l = 0; l < cfg->blocks; ++l) {
        FusedBlk& k = a.blk[l];
        const int p = 3 + 12 * l, o = SLAB_BLK0 + l * SLAB_BLK;
        k.wq = W(p); k.wk = W(p + 1); k.wv = W(p + 2); k.wfc = W(p + 3); k.ln1g = W(p + 4); k.ln1b = W(p + 5);
        k.w1 = W(p + 6); k.b1 = W(p + 7); k.w2 = W(p + 8); k.b2 = W(p + 9); k.ln2g = W(p + 10); k.ln2b = W(p + 11);
        k.Q = w.Q[l]; k.K = w.K[l]; k.V = w.V[l]; k.P = w.P[l]; k.C = w.C[l]; k.Zattn = w.Zattn[l]; k.X1 = w.X1[l];
        k.Hf = w.Hf[l]; k.Zffn = w.Zffn[l]; k.X2 = w.X2[l];
        add(p, o + SB_WQ, 4096); add(p + 1, o + SB_WK, 4096); add(p + 2, o + SB_WV, 4096); add(p + 3, o + SB_WFC, 4096);
        add(p + 4, o + SB_LN1G, 64); add(p + 5, o + SB_LN1B, 64); add(p + 6, o + SB_W1, 16384); add(p + 7, o + SB_B1, 256);
        add(p + 8, o + SB_W2, 16384); add(p + 9, o + SB_B2, 64); add(p + 10, o + SB_LN2G, 64); add(p + 11, o + SB_LN2B, 64);
    }
    a.slab = slab; a.slab_stride = SLAB_BLK0 + cfg->blocks * SLAB_BLK;
    a.B = B; a.S = cfg->seq; a.H = cfg->heads; a.blocks = cfg->blocks; a.G = FR / cfg->seq;
    const DropCfg d = make_drop(cfg->seed, 0, cfg->dropout);
    a.seed = d.seed; a.thr24 = d.thr24; a.inv_keep = d.inv_keep;
    const size_t lds = (size_t)(9 * FR * FLD + 2 * 192 * 16 + 512) * sizeof(float);
    const int nwg = (int)ceil_div(B, a.G);
    static OncePerDevice attr;
    if (attr.first()) {
        IISAN_HIP_OK(hipFuncSetAttribute((const void*)sasrec_fused_bwd_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        IISAN_HIP_OK(hipFuncSetAttribute((const void*)sasrec_fused_bwd_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        IISAN_HIP_OK(hipFuncSetAttribute((const void*)sasrec_fused_bwd_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    switch (FE / cfg->heads) {
        case 64: hipLaunchKernelGGL(sasrec_fused_bwd_kernel<64>, dim3(nwg), dim3(256), lds, s, a); break;
        case 32: hipLaunchKernelGGL(sasrec_fused_bwd_kernel<32>, dim3(nwg), dim3(256), lds, s, a); break;
        case 16: hipLaunchKernelGGL(sasrec_fused_bwd_kernel<16>, dim3(nwg), dim3(256), lds, s, a); break;
        default: iisan_set_error("sasrec_fused: head width %d not instantiated", FE / cfg->heads); return IISAN_EBADSHAPE;
    }
    IISAN_LAUNCH_OK();
    hipLaunchKernelGGL(sasrec_reduce_kernel, dim3(64, tab.n), dim3(256), 0, s, slab, a.slab_stride, nwg, tab);      // 64 x 256 threads: one element each of the largest tensors
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}
