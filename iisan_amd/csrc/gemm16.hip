// 16-bit-operand MFMA GEMM of the frozen encoders:  C = epilogue(A[M,K] · W[N,K]^T + bias), fp32 accumulate.
//
// This is where ≈96 % of the hot path's FLOPs go (QKV, O, FC1, FC2 and the patch-embedding
// conv-as-GEMM).  Roofline: bf16/f16 MFMA (2.5 PFLOP/s dense).  Structure (gfx950):
//   * 128x128x64 tile per 256-thread workgroup (4 waves as 2x2, 64x64 per wave = 4x4 fragments of
//     v_mfma_f32_16x16x32), two workgroups per CU;
//   * both operand tiles go HBM/L2 -> LDS with `global_load_lds_dwordx4` (no VGPR round trip), double buffered:
//     the DMA of K-tile t+1 is in flight while tile t feeds the MFMAs, one vmcnt(0)+barrier per K-tile;
//   * LDS tiles are row-major with 128-byte rows; 16-byte slots are XOR-swizzled with (row & 7) so the
//     ds_read_b128 fragment reads are bank-conflict free.  The DMA destination is lane-linear, so the swizzle is
//     applied to the per-lane SOURCE address and again on the read (guide §5.4 rule 21);
//   * operands are swapped in the MFMA (W rows as the "A" operand) and W rows are permuted while staging, so each
//     lane ends up with 8 CONSECUTIVE output columns of one row -> 16-byte (16-bit out) / 2x16-byte (fp32 out)
//     epilogue stores, bias/residual/GELU/position-embedding fused;
//   * logical tile ids are remapped per XCD so co-resident workgroups share A row panels in their L2.
#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;       // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;   // A + W
constexpr int RAG_N_END = 768;                // a ragged last column tile (N % 128 == 64) is served below this N (gemm16_route)

// RAG: N % 128 == 64 — the last column tile holds 64 live columns (the 192- and 576-column products of a 192-wide tower).  Its upper 64
// W rows do not exist and the weights may END there: the staging address of such a row is clamped to the last row of W (as attn16_dma.hip
// clamps its pad rows), so nothing is read past the allocation and the slots those lanes fill are never multiplied.  wave_n == 1 owns the
// dead columns: it stages and meets every barrier, skips its MFMAs (a wave-uniform branch), reads no bias and stores nothing.  A template
// flag, so that the whole-tile instantiations keep their instruction streams (profiles/narrow_towers.md).
template <typename T, int EPI, bool RAG = false>
__global__ __launch_bounds__(256, 2) void gemm16_kernel(Gemm16Args p) {
    static_assert(!RAG || EPI != EPI_F32, "EPI_F32 has its own ragged tile: its W image is padded to whole tiles");
    typedef typename T::v8 V8;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wave_m = wave >> 1, wave_n = wave & 1;

    const int tiles_n = (p.N + BN - 1) / BN;          // only EPI_F32 launches have a ragged last column tile
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_m = t / tiles_n, tile_n = t - tile_m * tiles_n;
    const int64_t m0 = (int64_t)tile_m * BM;
    const int n0 = tile_n * BN;

    const char* Ag = (const char*)p.A + m0 * p.lda * 2;
    const char* Wg = (const char*)p.W + (int64_t)n0 * p.ldw * 2;

    // staging: chunk c = wave*4+j covers LDS rows 8c..8c+7 (1 KiB); lane -> row q = 8c + (lane>>3), physical
    // 16-byte slot lane&7, which must hold logical slot (lane&7) ^ (q&7).
    int64_t a_off[4], w_off[4];
    {
        const int slog = (lane & 7) ^ (lane >> 3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = (wave * 4 + j) * 8 + (lane >> 3);
            a_off[j] = (int64_t)q * p.lda * 2 + slog * 16;
            int wq = nperm(q);
            if constexpr (RAG) wq = n0 + wq < p.N ? wq : p.N - 1 - n0;       // a row past the end of W: read its last row instead
            w_off[j] = (int64_t)wq * p.ldw * 2 + slog * 16;
        }
    }
    auto stage = [&](int kt, int buf) {
        char* sA = smem + buf * STAGE_BYTES + wave * 4096;
        char* sW = sA + TILE_BYTES;
        const int64_t kb = (int64_t)kt * (BK * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(Ag + a_off[j] + kb, sA + j * 1024);
#pragma unroll
        for (int j = 0; j < 4; ++j) glds16(Wg + w_off[j] + kb, sW + j * 1024);
    };

    f4 acc[4][2][2];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int a = 0; a < 2; ++a) acc[b][nb][a] = (f4){0.f, 0.f, 0.f, 0.f};

    // fragment read addresses: row = base + (lane&15) (so row&7 == lane&7), logical slot = kk*4 + (lane>>4)
    const int frow = lane & 15, fg = lane >> 4, fsw = lane & 7;
    const int xrow_off = (wave_m * 64 + frow) * 128;
    const int wrow_off = (wave_n * 64 + frow) * 128;
    const bool dead = RAG && n0 + wave_n * 64 >= p.N;      // wave-uniform: this wave's 64 columns lie beyond N

    int nk = p.K / BK, k_first = 0;
    if constexpr (EPI == EPI_F32) {                   // split-K: blockIdx.y owns a contiguous range of K-tiles
        // split-operand products: when one operand turned out exact in fp16 its lo plane (the last third of K) is zero;
        // the K-splits share what is left
        const int k_live = (p.skip_last_third && p.skip_last_third[0] == 0) ? nk / 3 * 2 : nk;
        const int per = (k_live + (int)gridDim.y - 1) / (int)gridDim.y;
        k_first = (int)blockIdx.y * per;
        int k_end = k_first + per;
        if (k_end > k_live) k_end = k_live;
        nk = k_end - k_first;
        if (nk < 0) nk = 0;                           // nothing to multiply: the epilogue still writes this split's zeros
    }
    if (nk > 0) stage(k_first, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) stage(k_first + kt + 1, cur ^ 1);
        const char* sA = smem + cur * STAGE_BYTES;
        const char* sW = sA + TILE_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            if (RAG && dead) break;                        // (no fragment reads, no MFMAs: the accumulators stay zero and are never stored)
            const int slot = ((kk * 4 + fg) ^ fsw) << 4;
            V8 xf[4], wf[2][2];
#pragma unroll
            for (int b = 0; b < 4; ++b) xf[b] = *(const V8*)(sA + xrow_off + b * 2048 + slot);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int a = 0; a < 2; ++a) wf[nb][a] = *(const V8*)(sW + wrow_off + (nb * 32 + a * 16) * 128 + slot);
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                    for (int a = 0; a < 2; ++a) acc[b][nb][a] = T::mfma(wf[nb][a], xf[b], acc[b][nb][a]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // ---- epilogue: lane (j = lane&15, g = lane>>4) owns row m0+wave_m*64+b*16+j, columns n..n+7 -----------------
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int64_t m = m0 + wave_m * 64 + b * 16 + frow;
        if (m >= p.M) continue;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            const int n = n0 + wave_n * 64 + nb * 32 + 8 * fg;
            if constexpr (RAG) {
                if (n + 8 > p.N) continue;                 // N % 8 == 0: a lane's 8 columns are all in or all out (no bias read either)
            }
            float v[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[b][nb][0][r];
                v[4 + r] = acc[b][nb][1][r];
            }
            if constexpr (EPI == EPI_F32) {
                if (n + 8 > p.N) continue;             // N % 8 == 0: a lane's 8 columns are all in or all out
                const float ia = p.inv_a ? p.inv_a[0] : 1.f, ib = p.inv_b ? p.inv_b[0] : 1.f;
#pragma unroll
                for (int r = 0; r < 8; ++r) v[r] = v[r] * ia * ib;
                float* op = (float*)p.out + (int64_t)blockIdx.y * p.split_stride + m * p.ldo + n;
                const bool first = gridDim.y == 1 || p.atomic;    // split-K partial products: bias / residual are the reducer's
                if (p.bias && first && (blockIdx.y == 0)) {
                    const f4 b0 = *(const f4*)(p.bias + n), b1 = *(const f4*)(p.bias + n + 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { v[r] += b0[r]; v[4 + r] += b1[r]; }
                }
                if (p.resid && first && (blockIdx.y == 0)) {
                    const float* rp = p.resid + m * p.ldo + n;
                    const f4 r0 = *(const f4*)rp, r1 = *(const f4*)(rp + 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r) { v[r] += r0[r]; v[4 + r] += r1[r]; }
                }
                if (p.atomic) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) unsafeAtomicAdd(op + r, v[r]);
                } else {
                    *(f4*)op = (f4){v[0], v[1], v[2], v[3]};
                    *(f4*)(op + 4) = (f4){v[4], v[5], v[6], v[7]};
                }
                continue;
            }
            if (p.bias) {
                const f4 b0 = *(const f4*)(p.bias + n), b1 = *(const f4*)(p.bias + n + 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] += b0[r];
                    v[4 + r] += b1[r];
                }
            }
            if constexpr (EPI == EPI_OUT16 || EPI == EPI_GELU16 || EPI == EPI_QGELU16 || EPI == EPI_QKVH16 || EPI == EPI_PATCH16) {
                V8 o;
#pragma unroll
                for (int r = 0; r < 8; ++r) o[r] = T::from_f32(EPI == EPI_GELU16 ? gelu_erf_fast(v[r]) : EPI == EPI_QGELU16 ? quick_gelu(v[r]) : v[r]);
                if constexpr (EPI == EPI_QKVH16) {
                    const int Dm = p.qkv_heads * 64;
                    const int64_t item = m / p.qkv_S;
                    const int tok = (int)(m - item * p.qkv_S);
                    const int wq_ = n / Dm, hd = (n - wq_ * Dm) >> 6, d = n & 63, which = wq_ + p.qkv_which0;
                    *(V8*)((typename T::elem*)p.out + (((item * p.qkv_heads + hd) * 3 + which) * p.qkv_S + tok) * 64 + d) = o;
                } else if constexpr (EPI == EPI_PATCH16) {
                    *(V8*)((typename T::elem*)p.out + (m + m / p.patch_P + 1) * p.ldo + n) = o;
                } else {
                    *(V8*)((typename T::elem*)p.out + m * p.ldo + n) = o;
                }
            } else if constexpr (EPI == EPI_RESID32) {
                const float* rp = p.resid + m * p.ldo + n;
                const f4 r0 = *(const f4*)rp, r1 = *(const f4*)(rp + 4);
                float* op = (float*)p.out + m * p.ldo + n;
                *(f4*)op = (f4){v[0] + r0[0], v[1] + r0[1], v[2] + r0[2], v[3] + r0[3]};
                *(f4*)(op + 4) = (f4){v[4] + r1[0], v[5] + r1[1], v[6] + r1[2], v[7] + r1[3]};
            } else {  // EPI_PATCH32: patch row m of image m/P -> token row img*(P+1)+1+m%P, + position embedding
                const int64_t img = m / p.patch_P;
                const int pp = (int)(m - img * p.patch_P);
                const float* pe = p.pos + (int64_t)(1 + pp) * p.N + n;
                const f4 r0 = *(const f4*)pe, r1 = *(const f4*)(pe + 4);
                float* op = (float*)p.out + (img * (p.patch_P + 1) + 1 + pp) * p.ldo + n;
                *(f4*)op = (f4){v[0] + r0[0], v[1] + r0[1], v[2] + r0[2], v[3] + r0[3]};
                *(f4*)(op + 4) = (f4){v[4] + r1[0], v[5] + r1[1], v[6] + r1[2], v[7] + r1[3]};
            }
        }
    }
}

template <typename T>
int launch_t(int mode, const Gemm16Args& a, hipStream_t s) {
    const int64_t tiles = ceil_div(a.M, BM) * ceil_div(a.N, BN);
    dim3 grid((unsigned)tiles), block(256);
    const bool rag = a.N % BN != 0;       // (gemm16_route: N % 128 == 64 then)
#define V1_CASE(E)                                                                                                             \
    case E:                                                                                                                    \
        if (rag) hipLaunchKernelGGL((gemm16_kernel<T, E, true>), grid, block, 0, s, a);                                        \
        else hipLaunchKernelGGL((gemm16_kernel<T, E>), grid, block, 0, s, a);                                                  \
        break
    switch (mode) {
        V1_CASE(EPI_OUT16); V1_CASE(EPI_GELU16); V1_CASE(EPI_RESID32); V1_CASE(EPI_PATCH32); V1_CASE(EPI_QKVH16); V1_CASE(EPI_PATCH16); V1_CASE(EPI_QGELU16);
        default: iisan_set_error("gemm16: bad epilogue mode %d", mode); return IISAN_EBADSHAPE;
    }
#undef V1_CASE
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

}  // namespace

// fp32-output launch of the 128x128 kernel for the split-operand GEMM (split.hip): fp16 operand images, optional split-K
// with atomic accumulation, ragged N (multiple of 8; the W image is padded to whole tiles).  Not timed by iisan_timing_*:
// that measures the frozen encoders' GEMMs only.
int launch_gemm16_f32(const Gemm16Args& a, int ksplit, hipStream_t s) {
    IISAN_CHECK_SHAPE(a.M > 0 && a.N > 0 && a.K > 0 && a.K % BK == 0 && a.N % 8 == 0 && a.ldo % 4 == 0, "gemm16_f32: bad shape");
    IISAN_CHECK_SHAPE(ksplit >= 1 && (ksplit == 1 || a.atomic || a.split_stride > 0), "gemm16_f32: split-K needs a partial-product buffer");
    IISAN_CHECK_SHAPE(!a.a_blk32 && !a.out_blk32, "gemm16_f32: block-major (blk32) operands run on gemm16_h256 only");
    const int64_t tiles = ceil_div(a.M, BM) * ceil_div(a.N, BN);
    IISAN_CHECK_SHAPE(tiles < (1ll << 31), "gemm16_f32: grid too large");
    hipLaunchKernelGGL((gemm16_kernel<F16, EPI_F32>), dim3((unsigned)tiles, (unsigned)ksplit), dim3(256), 0, s, a);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

// The shape of the extern "C" entries below — A [M, K], W [N, K] and out [M, N] with their natural leading dimensions — and the
// two layout flags of the block-major intermediates (DEV section; in the product only the encoder executors set them)
static Gemm16Args natural_args(int64_t M, int32_t N, int32_t K, int32_t a_blk32, int32_t out_blk32) {
    Gemm16Args a{};
    a.M = M; a.N = N; a.K = K; a.lda = K; a.ldw = K; a.ldo = N;
    a.a_blk32 = a_blk32 != 0; a.out_blk32 = out_blk32 != 0;
    return a;
}

// bench / test entry: fp16 operands [M,K] x [N,K]^T -> fp32 out (plain or split-K with atomics into a caller-zeroed out)
extern "C" int iisan_gemm16_f32(const void* A, const void* W, float* out, int64_t M, int32_t N, int32_t K, int32_t ksplit,
                                void* stream) {
    Gemm16Args a = natural_args(M, N, K, 0, 0);
    a.A = A; a.W = W; a.out = out;
    a.atomic = ksplit > 1 ? 1 : 0;
    return launch_gemm16_f32(a, ksplit, (hipStream_t)stream);
}

// 0 = auto (persistent 256x256 kernels when the shape allows and there is at least half a tile per CU), 1 and 2 = force the
// 128x128 v1 kernel, 3 = force the staggered 256x256 kernel (gemm16_s256.hip), 4 = force the staggered kernel with the half-slot
// tile boundary (gemm16_h256.hip).
// Test/bench knob, not part of the product ABI.
static int g_variant = 0;
// auto policy: gemm16_h256.hip takes the production shapes (half-slot tile boundary: same-box A/B of tools/gemm_var.py over three
// boxes against gemm16_s256.hip: QKV +1..4 %, O +1 %, FC1 +-0, FC2 +3..4 %; bit-identical results); variant 3 still forces
// gemm16_s256.hip for the race screen
IISAN_DEV_KNOB(gemm16_variant, g_variant);
static int64_t g_cnt_h256 = 0, g_cnt_s256 = 0, g_cnt_v1 = 0;      // launches of launch_gemm16 by kernel family
IISAN_DEV_COUNTER(gemm16_h256, g_cnt_h256);
IISAN_DEV_COUNTER(gemm16_s256, g_cnt_s256);
IISAN_DEV_COUNTER(gemm16_v1, g_cnt_v1);
static int64_t g_cnt_blk32 = 0;       // ... of them, gemm16_h256 launches with a block-major operand or output (Gemm16Args::a_blk32 / out_blk32)
IISAN_DEV_COUNTER(gemm16_blk32, g_cnt_blk32);
// tile walk of gemm16_h256 (bench knob): c = -1 auto policy, 0 = row-major tile list, > 0 = panels of c column tiles walked down
// sub-slabs of h row tiles (h <= 0: the XCD's whole slab)
static int g_walk_c = -1, g_walk_h = 0;
IISAN_DEV_KNOB(gemm16_walk_c, g_walk_c);
IISAN_DEV_KNOB(gemm16_walk_h, g_walk_h);

static int reject(const char* what, int mode, const Gemm16Args& a) {
    iisan_set_error("gemm16: %s (mode %d, M=%lld N=%d K=%d, variant %d)", what, mode, (long long)a.M, a.N, a.K, g_variant & 0xff);
    return G16_REJECTED;
}

int gemm16_route(int dtype16, int mode, const Gemm16Args& a) {
    if (mode < EPI_OUT16 || mode > EPI_QGELU16 || mode == EPI_F32) return reject("bad epilogue mode", mode, a);     // (EPI_F32: launch_gemm16_f32)
    if (!(a.M > 0 && a.N > 0 && a.K > 0)) return reject("empty problem", mode, a);
    // N % 128 == 64 below RAG_N_END: a ragged last column tile, on the 128x128 kernel alone (both 256x256 kernels turn down N % 256 != 0) — the
    // 192- and 576-column products of a 192-wide tower.  From 768 columns on every supported width is a multiple of 128 and a ragged N is refused
    if (!((a.N % BN == 0 || (a.N % 64 == 0 && a.N < RAG_N_END)) && a.K % BK == 0))
        return reject("N must be a multiple of 128 (below 768: of 64) and K of 64", mode, a);
    if (!(ceil_div(a.M, BM) * ceil_div(a.N, BN) < (1ll << 31))) return reject("grid too large", mode, a);
    if (mode == EPI_PATCH32 && !(a.patch_P > 0 && a.pos)) return reject("patch mode needs P and pos", mode, a);
    if (mode == EPI_PATCH16 && !(a.patch_P > 0)) return reject("patch mode needs P", mode, a);
    if (mode == EPI_RESID32 && !a.resid) return reject("residual mode needs resid", mode, a);
    if (mode == EPI_STREAM16 && !(a.rowpart && a.qkv_S > 0 && a.ldo == a.N)) return reject("stream mode needs the row-sum buffer, S and ldo == N", mode, a);
    if (mode == EPI_QKVH16 && !(a.qkv_S > 0 && a.qkv_heads > 0 && a.qkv_which0 >= 0 && a.qkv_which0 <= 2 && a.N == (3 - a.qkv_which0) * 64 * a.qkv_heads))
        return reject("head-major QKV mode needs S, heads and N == (3 - which0)*64*heads", mode, a);
    const int var = g_variant & 0xff;
    // the 256x256 kernels: forced (variants 3, 4), or where there is at least half a tile per CU (auto)
    const bool big = var == 3 || var == 4 || (var == 0 && ceil_div(a.M, 256) * (a.N / 256) >= 128);
    const bool h256 = big && var != 3 && gemm16_h256_applicable(mode, a);
    // LayerNorm in the epilogue and the stream epilogue exist on gemm16_h256 alone, with fp16 operands
    if (mode == EPI_STREAM16 || a.rowstat) {
        if (!h256) return reject(a.rowstat ? "a product with LayerNorm row statistics runs on gemm16_h256 only" : "the stream epilogue runs on gemm16_h256 only", mode, a);
        if (dtype16 != IISAN_F16) return reject("row statistics and the stream epilogue need fp16 operands", mode, a);
    }
    // block-major intermediates (Gemm16Args::a_blk32 / out_blk32) exist on gemm16_h256 alone: never read or written row-major by mistake
    if ((a.a_blk32 || a.out_blk32) && !h256) return reject("block-major (blk32) operands run on gemm16_h256 only, FC1 output / FC2 A operand", mode, a);
    if (h256) return G16_H256;
    // the staggered kernel without the half-slot boundary: variant 3 (the race-screen reference of gemm16_h256) and the shapes
    // gemm16_h256_applicable() turns down (it has no EPI_QGELU16: under variant 3 that mode goes on to the 128x128 kernel)
    if (big && var != 4 && gemm16_s256_applicable(mode, a)) return G16_S256;
    // everything else — small shapes, the fp32 / residual epilogues — on the 128x128 kernel
    return G16_V1;
}

int launch_gemm16(int dtype16, int mode, const Gemm16Args& a, hipStream_t s) {
#ifndef GEMM16_DEBUG_BITS
    // ablation / experiment bits (gemm16_variant = 4 | bits << 8) exist only in `make EXTRA=-DGEMM16_DEBUG_BITS` builds: a default
    // build would run the plain product kernel and the A/B tools (tools/gemm_walk.py, gemm_stream.py, gemm_slots_h.py) would read
    // numbers that mean nothing
    IISAN_CHECK_SHAPE((g_variant >> 8) == 0, "gemm16: debug bits 0x%x requested, but this library was built without -DGEMM16_DEBUG_BITS", (unsigned)(g_variant >> 8));
#endif
    const int route = gemm16_route(dtype16, mode, a);
    if (route == G16_REJECTED) return IISAN_EBADSHAPE;
    TimedLaunch timed(1, s, 2.0 * (double)a.M * a.N * a.K, 2.0 * ((double)a.M * a.K + (double)a.N * a.K + (double)a.M * a.N));
    Gemm16Args b = a;
    switch (route) {
        case G16_H256:
            b.debug = g_variant >> 8;
            {   // auto policy (tools/gemm_walk.py, three boxes, interleaved rounds: QKV 1,010 -> 1,045, FC1 972 -> 990 TFLOP/s; the L2 read
                // latency seen by the L1 falls from 396 to 239 cycles, profiles/r4_gemm_l2.md): panels of 3 column tiles walked down
                // sub-slabs of 16 row tiles wherever a tile row is at least two panels wide and every XCD's slab holds a few sub-slabs
                const bool auto_panel = a.N / 256 >= 6 && ceil_div(a.M, 256) >= 128;
                b.walk_c = g_walk_c < 0 ? (auto_panel ? 3 : 0) : g_walk_c;
                b.walk_h = g_walk_c < 0 ? 16 : g_walk_h;
            }
            ++g_cnt_h256;
            if (a.a_blk32 || a.out_blk32) ++g_cnt_blk32;
            return launch_gemm16_h256(dtype16, mode, b, s);
        case G16_S256:
            b.debug = g_variant >> 8;
            ++g_cnt_s256;
            return launch_gemm16_s256(dtype16, mode, b, s);
        default:
            ++g_cnt_v1;
            return dtype16 == IISAN_BF16 ? launch_t<BF16>(mode, a, s) : launch_t<F16>(mode, a, s);
    }
}

// The entries that come in pairs: NAME_blk32 carries the two layout flags of the block-major ("blk32") intermediates (DEV section;
// tests/test_gpu_blk32.py, tools/gemm_blk32_ab.py), NAME is the same call with both flags off.

// the routing query for host-side tests (tests/test_host_logic.py): operands with natural leading dimensions, qkv_S doubles as the
// patch count of EPI_PATCH16, non-null placeholders for the buffers the checks ask for; no device is touched
extern "C" int32_t iisan_gemm16_route_blk32(int32_t dtype16, int32_t mode, int64_t M, int32_t N, int32_t K, int32_t qkv_S, int32_t qkv_heads,
                                            int32_t qkv_which0, int32_t with_rowstat, int32_t a_blk32, int32_t out_blk32) {
    static float dummy = 0.f;
    Gemm16Args a = natural_args(M, N, K, a_blk32, out_blk32);
    a.qkv_S = qkv_S; a.qkv_heads = qkv_heads; a.qkv_which0 = qkv_which0;
    a.patch_P = mode == EPI_PATCH16 || mode == EPI_PATCH32 ? qkv_S : 0;
    a.rowstat = with_rowstat ? &dummy : nullptr;
    a.rowpart = &dummy; a.resid = &dummy; a.pos = &dummy;
    return gemm16_route(dtype16, mode, a);
}
extern "C" int32_t iisan_gemm16_route(int32_t dtype16, int32_t mode, int64_t M, int32_t N, int32_t K, int32_t qkv_S, int32_t qkv_heads,
                                      int32_t qkv_which0, int32_t with_rowstat) {
    return iisan_gemm16_route_blk32(dtype16, mode, M, N, K, qkv_S, qkv_heads, qkv_which0, with_rowstat, 0, 0);
}

// bench / test entry: x += A W^T + bias in the fp16 stream x [Mpad, N] (in place), per-slice row sums into rowpart [N / 64][Mpad][2]
extern "C" int iisan_gemm16_stream_blk32(const void* A, const void* W, const float* bias, void* x16, float* rowpart, int64_t M, int32_t N,
                                         int32_t K, int32_t S, int32_t a_blk32, int32_t x_blk32, void* stream) {
    Gemm16Args a = natural_args(M, N, K, a_blk32, x_blk32);
    a.A = A; a.W = W; a.bias = bias; a.out = x16; a.rowpart = rowpart; a.qkv_S = S;
    return launch_gemm16(IISAN_F16, EPI_STREAM16, a, (hipStream_t)stream);
}
extern "C" int iisan_gemm16_stream(const void* A, const void* W, const float* bias, void* x16, float* rowpart, int64_t M, int32_t N,
                                   int32_t K, int32_t S, void* stream) {
    return iisan_gemm16_stream_blk32(A, W, bias, x16, rowpart, M, N, K, S, 0, 0, stream);
}

// ... and the finalize step behind it
extern "C" int iisan_stream_stats_finalize_blk32(const float* rowpart, int32_t nslots, int64_t Mpad, void* x16, float* xc, float* rstat, float eps,
                                                 int64_t items, int32_t Ttok, int32_t x_blk32, void* stream) {
    return launch_stream_stats_finalize(rowpart, nslots, Mpad, x16, xc, rstat, eps, items, Ttok, (hipStream_t)stream, x_blk32 != 0);
}
extern "C" int iisan_stream_stats_finalize(const float* rowpart, int32_t nslots, int64_t Mpad, void* x16, float* xc, float* rstat, float eps,
                                           int64_t items, int32_t Ttok, void* stream) {
    return iisan_stream_stats_finalize_blk32(rowpart, nslots, Mpad, x16, xc, rstat, eps, items, Ttok, 0, stream);
}

// bench / test entry (not in the product ABI): LN(x) W^T + b with the LayerNorm applied in the epilogue — A = x [M, K] fp16,
// W = the folded weights, rowstat [Mpad] (null: plain product); mode 1 (GELU) or 4 (head-major QKV: S tokens per item, N / 192 heads)
extern "C" int iisan_gemm16_lna(int32_t mode, const void* A, const void* W, const float* bias, void* out, const float* rowstat,
                                int64_t M, int32_t N, int32_t K, int32_t S, void* stream) {
    Gemm16Args a = natural_args(M, N, K, 0, 0);
    a.A = A; a.W = W; a.bias = bias; a.out = out; a.rowstat = rowstat;
    if (mode == EPI_QKVH16) { a.qkv_S = S; a.qkv_heads = N / 192; }
    return launch_gemm16(IISAN_F16, mode, a, (hipStream_t)stream);
}

// DEV-section entry of the block-major intermediates: the product of iisan_gemm16 (modes 0 / 1 / 8; rowstat != null: LayerNorm in the
// epilogue, fp16) with the two layout flags
extern "C" int iisan_gemm16_blk32(int32_t dtype16, int32_t mode, const void* A, const void* W, const float* bias, void* out,
                                  const float* rowstat, int64_t M, int32_t N, int32_t K, int32_t a_blk32, int32_t out_blk32, void* stream) {
    IISAN_CHECK_SHAPE(mode == EPI_OUT16 || mode == EPI_GELU16 || mode == EPI_QGELU16, "iisan_gemm16_blk32: mode must be 0, 1 or 8");
    Gemm16Args a = natural_args(M, N, K, a_blk32, out_blk32);
    a.A = A; a.W = W; a.bias = bias; a.out = out; a.rowstat = rowstat;
    return launch_gemm16(dtype16, mode, a, (hipStream_t)stream);
}

// bench / test entry: the weight fold of one LayerNorm + product pair (rowops.hip)
extern "C" int iisan_fold_ln_weights(const void* W, int32_t w32, const float* bias, const float* g, const float* b, void* Wf, float* bf,
                                     int32_t N, void* stream) {
    LnFoldJob j{W, bias, g, b, Wf, bf, N, w32};
    return launch_fold_ln_weights(&j, 1, (hipStream_t)stream);
}

extern "C" int iisan_gemm16(int32_t dtype16, int32_t mode, const void* A, const void* W, const float* bias, void* out,
                            const float* resid, int64_t M, int32_t N, int32_t K, void* stream) {
    IISAN_CHECK_SHAPE((mode >= 0 && mode <= 2) || mode == EPI_QGELU16, "iisan_gemm16: mode must be 0, 1, 2 or 8");
    Gemm16Args a = natural_args(M, N, K, 0, 0);
    a.A = A; a.W = W; a.bias = bias; a.out = out; a.resid = resid;
    return launch_gemm16(dtype16, mode, a, (hipStream_t)stream);
}

// bench entry (not in the product ABI): the same product with explicit leading dimensions (elements) — tools/gemm_ld.py
// asks whether the row stride of the operands (1536 B at K = 768) costs L2 channel parallelism.
extern "C" int iisan_gemm16_ld(int32_t dtype16, int32_t mode, const void* A, const void* W, const float* bias, void* out,
                               int64_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldo, void* stream) {
    IISAN_CHECK_SHAPE((mode >= 0 && mode <= 1) || mode == EPI_QGELU16, "iisan_gemm16_ld: mode must be 0, 1 or 8");
    Gemm16Args a{};
    a.A = A; a.W = W; a.bias = bias; a.out = out;
    a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldo = ldo;
    return launch_gemm16(dtype16, mode, a, (hipStream_t)stream);
}
