// Fused in-batch debiased cross-entropy (forward + backward) — the [T, M] logits matrix is never materialised.
// Replaces the loss section of ModelMM.forward (Code_Uncached/model/model.py:81-104), including its O(bs)
// Python masking loop (model.py:92-100) whose autograd graph dominates the reference's Cached step at bs=1024
// (SURVEY.md §3.2).  Exact semantics kept, in the reference's order:
//     z[row,c]  = prec[row]·score[c] - log pop[id_c]
//     z[:,c]    = -1e4   if slot c is history padding (position < S and log_mask == 0)            (model.py:88-89)
//     z[row,c]  = -1e4   if id_c occurs in the row's own sequence and c is not the row's positive  (model.py:92-100)
//     loss      = mean over rows with log_mask != 0 of  logsumexp(z[row,:]) - z[row, label]       (model.py:102-104)
// The -1e4 are ASSIGNED: a filled logit is a constant.  The false-negative fill spares the label, the padding fill does not — a label
// column with log_mask == 0 (a hole in the mask; never with left padding) is -1e4 in the loss and carries no gradient.
//
// Three families of kernels compute it (ce_route below says which one a call takes):
//     ce_pass_kernel                          the plain statement of the loss, any shape
//     ce_rowpass_kernel / ce_colpass_kernel   the same walk with the per-logit work done once per wave and tile (5 <= S <= 15)
//     ce16_*                                  split fp16 operands on the 16-bit matrix cores (large batches)
//
// THE LAYOUT OF THE f32 PASSES (the first two families; stated here once).  A pass fixes 16 rows of X per workgroup (prec rows for
// the forward and d_prec, score rows for d_score) and streams the other matrix Y in 16-row tiles, its four waves taking tiles
// round-robin.  Logit tiles are computed TRANSPOSED on the f32 matrix cores (v_mfma_f32_16x16x4_f32, K = E = 64): lane (j, g) =
// (lane & 15, lane >> 4) owns X row x0 + j and the Y rows y0 + 4g .. 4g + 3 of the tile.  So the online log-sum-exp is per lane plus
// two xor-shuffles (16, 32), and the four dZ registers of a lane are already the B operand of the second product dX^T += Y^T·dZ^T,
// whose accumulators dacc[et][r] hold dX[x0 + j][16 et + 4g + r].  A wave stages its Y tile in LDS once, rows of E + 4 = 68 floats
// (272 bytes: conflict-free ds_read_b128); both products read their A operand from it, the second one transposed.  The four waves'
// results meet in sRed after the walk.  The passes are templates over the width EW = 64 NE (NE = 1 .. 4 feature blocks of 64): K = EW,
// rows of EW + 4 floats (4 mod 64 at every width: the same bank walk), 4 NE accumulators; what is said of E = 64 here is the NE = 1 case.
#include <type_traits>

#include "common.h"

namespace {

constexpr int E = 64;             // the width of the split-operand route (ce16_*) and of the calls without a width argument
constexpr int EMAX = 256;         // the f32 passes are instantiated at EW = 64, 128, 192, 256: NE = EW / 64 feature blocks of 64
constexpr int MAXS1 = 16;         // sequences of up to 16 slots keep their ids in registers / LDS (longer ones take the plain kernel)
constexpr float MASKV = -1e4f;

struct CeBufs {
    int* ids32;      // [M]
    float* debias;   // [M] log pop[id]
    int* colpad;     // [M] 1 if the slot is history padding
    float* lse;      // [T]
    float* rowloss;  // [T]
    float* nvalid;   // [1]
    float* dprec;    // [T, E] d loss / d prec for d_loss = 1, left by the fused forward pass (ce_rowpass_kernel<CE_FUSED>)
};

void carve(WsCarver& c, CeBufs& b, int64_t bs, int S, int EW) {
    const size_t M = (size_t)bs * (S + 1), T = (size_t)bs * S;
    b.ids32 = c.take<int>(M);
    b.debias = c.take<float>(M);
    b.colpad = c.take<int>(M);
    b.lse = c.take<float>(T);
    b.rowloss = c.take<float>(T);
    b.nvalid = c.take<float>(4);
    b.dprec = c.take<float>(T * EW);
}

__global__ void ce_prep_kernel(const int64_t* __restrict__ ids, const float* __restrict__ log_mask,
                               const float* __restrict__ pop, int64_t n_pop, CeBufs b, int64_t bs, int S) {
    const int64_t M = bs * (S + 1);
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < M; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = c / (S + 1);
        const int p = (int)(c - i * (S + 1));
        const int64_t id = ids[c];
        b.ids32[c] = (int)id;
        b.debias[c] = (id >= 0 && id < n_pop) ? logf(pop[id]) : __builtin_nanf("");     // bad id: loud NaN loss, no wild read
        b.colpad[c] = (p < S && log_mask[i * S + p] == 0.f) ? 1 : 0;
    }
}

// sum of one value per thread of a 256-thread workgroup, in a fixed order (a tree over the thread index); the result is thread 0's
__device__ __forceinline__ float block_sum256(float s) {
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// n_valid = #{log_mask != 0}; single block, fixed order
__global__ __launch_bounds__(256) void ce_count_kernel(const float* __restrict__ log_mask, int64_t T, float* out) {
    float s = 0.f;
    // (16-byte loads, all of a thread's requests in flight: one dependent 4-byte load per iteration made this single-workgroup pass 10.7 us at T = 10,240;
    //  the counts are small integers: any summation order is exact)
    const int64_t T4 = (T % 4 == 0 && ((uintptr_t)log_mask & 15) == 0) ? T / 4 : 0;
    for (int64_t i = threadIdx.x; i < T4; i += 256) {
        const f4 v = ((const f4*)log_mask)[i];
        s += (v[0] != 0.f ? 1.f : 0.f) + (v[1] != 0.f ? 1.f : 0.f) + (v[2] != 0.f ? 1.f : 0.f) + (v[3] != 0.f ? 1.f : 0.f);
    }
    for (int64_t i = 4 * T4 + threadIdx.x; i < T; i += 256) s += log_mask[i] != 0.f ? 1.f : 0.f;
    s = block_sum256(s);
    if (threadIdx.x == 0) out[0] = s;
}

// loss = sum of the row losses / n_valid; single block
__global__ __launch_bounds__(256) void ce_reduce_kernel(const float* __restrict__ rowloss, int64_t T, const float* nvalid,
                                                        float* loss) {
    float s = 0.f;
    // 16-byte loads (as ce_count_kernel); the order is fixed — thread t adds the groups t, t + 256, ... of four rows, each as (r0 + r1) + (r2 + r3)
    const int64_t T4 = (T % 4 == 0 && ((uintptr_t)rowloss & 15) == 0) ? T / 4 : 0;
    for (int64_t i = threadIdx.x; i < T4; i += 256) {
        const f4 v = ((const f4*)rowloss)[i];
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    for (int64_t i = 4 * T4 + threadIdx.x; i < T; i += 256) s += rowloss[i];
    s = block_sum256(s);
    if (threadIdx.x == 0) loss[0] = s / nvalid[0];
}

// ---------------------------------------------------------------------------------------------------------------------
// The pieces the three f32 passes are written over (layout: top of the file).  Index types are the caller's: `int` in the row-fixed
// kernels (M < 2^31 is their launch condition), int64_t in the plain one; an address is widened where EW multiplies it.  Every
// floating-point expression below is evaluated in this order by every pass: the routes agree to the bit wherever they share one.
// EW is the embedding width, NE = EW / 64: feature 64 nb + 16 g + 4 v + e is K-step (nb, v, e) of lane group g in the logits product,
// and feature block et = 4 nb + .. of the second one — at EW = 64 the pieces are the code they were before they took a width.
enum { CE_FWD = 0, CE_DPREC = 1, CE_DSCORE = 2, CE_FUSED = 3 };
template <int EW>
using CeRed = float[4][16][EW + 4];     // per wave and X row: EW features (+ m, l, z_label of the fused finish)
// The planes the four waves' results meet in.  A wave's plane is as large as its Y tile (16 rows of EW + 4 floats), and a wave is done
// with its tile when it writes its plane: at EW > 64 the planes ARE the tiles (66.6 KB of LDS instead of 133 KB at EW = 256: two
// workgroups per CU, as many as its registers allow; profiles/wide_embedding.md).  EW = 64 keeps planes of its own (34.8 KB with the
// tiles, four workgroups per CU either way).
template <int EW>
using CeRedOwn = std::conditional_t<(EW > 64), float[4], CeRed<EW>>;
template <int EW>
__device__ __forceinline__ CeRed<EW>& ce_red(float (&sY)[4][16 * (EW + 4)], CeRedOwn<EW>& own) {
    if constexpr (EW > 64) return *reinterpret_cast<CeRed<EW>*>(&sY[0][0]);
    else return own;
}

// exp(x) = v_exp_f32(x * log2 e): 2 instructions.  The product is rounded once, so the relative error is |x| 2^-24 plus the ulp of
// v_exp_f32 — and every argument here is a logit minus a maximum or an lse, <= 0 up to rounding: a term that far below the top weighs
// e^-|x|, its share of the error of a sum is |x| e^-|x| 2^-24 <= 2.2e-8 at ANY |x|.  tests/test_gpu_ce_regimes.py runs arguments from 0
// down to -300 (logits of +-150) next to the -1e4 fills, which underflow to 0 exactly as with expf: loss within 2.1e-6 and gradients
// within 4.7e-6 of the float64 oracle on every route (profiles/ce_regimes.md; the bounds are 2e-5 and 2e-4)
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// the label column of prec row x: the next slot of its sequence (S rows, S + 1 columns per sequence)
template <class I>
__device__ __forceinline__ I ce_label(I x, int S) {
    const I seq = x / S;
    return seq * (S + 1) + (x - seq * S) + 1;
}

__device__ __forceinline__ bool id_in_seq(const int* __restrict__ ids32, int64_t seq, int S1, int idc) {
    bool hit = false;
    for (int p = 0; p < S1; ++p) hit |= ids32[seq * S1 + p] == idc;
    return hit;
}

// X fragments of row xc (B operand of the logits product): e(ks, kq) = 16*kq + ks -> 16 consecutive floats per lane
template <int EW>
__device__ __forceinline__ void ce_load_x(float (&xb)[EW / 4], const float* __restrict__ X, int64_t xc, int g) {
#pragma unroll
    for (int nb = 0; nb < EW / 64; ++nb)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const f4 t = *(const f4*)(X + xc * EW + 64 * nb + 16 * g + 4 * v);
#pragma unroll
            for (int e = 0; e < 4; ++e) xb[16 * nb + 4 * v + e] = t[e];
        }
}

// the wave's Y tile from registers into LDS: 16 rows x EW floats, lane -> row lane >> 2, 16-float chunk lane & 3 of every feature block
// (ce_ypart: where lane's piece (nb, v) of row yr sits in global memory)
template <int EW>
__device__ __forceinline__ const float* ce_ypart(const float* __restrict__ Y, int64_t yr, int lane, int nb, int v) {
    return Y + yr * EW + 64 * nb + (lane & 3) * 16 + v * 4;
}
template <int EW>
__device__ __forceinline__ void ce_stage_y(float* myY, const f4 (&yreg)[EW / 16], int lane) {
    const int r = lane >> 2, ch = lane & 3;
#pragma unroll
    for (int nb = 0; nb < EW / 64; ++nb)
#pragma unroll
        for (int v = 0; v < 4; ++v) *(f4*)(myY + r * (EW + 4) + 64 * nb + ch * 16 + v * 4) = yreg[4 * nb + v];
}

// Z^T tile: A = Y rows (i = lane & 15), B = X rows; the lane receives z(x0 + j, y0 + 4g + r).  Two independent accumulator chains
// (a single one is 16 MFMAs each waiting for the previous result)
template <int EW>
__device__ __forceinline__ f4 ce_logits(const float* myY, const float (&xb)[EW / 4], int j, int g) {
    f4 z = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int nb = 0; nb < EW / 64; ++nb)
#pragma unroll
        for (int v = 0; v < 4; v += 2) {
            const f4 ya = *(const f4*)(myY + j * (EW + 4) + 64 * nb + 16 * g + 4 * v);
            const f4 yb = *(const f4*)(myY + j * (EW + 4) + 64 * nb + 16 * g + 4 * v + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                z = __builtin_amdgcn_mfma_f32_16x16x4f32(ya[e], xb[16 * nb + 4 * v + e], z, 0, 0, 0);
                z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(yb[e], xb[16 * nb + 4 * v + 4 + e], z1, 0, 0, 0);
            }
        }
    z += z1;
    return z;
}

// dX^T[e][x] += sum_y Y[y][e] dZ(x, y):  A = Y^T (i = e within feature block et, k = y0 + 4kq + r), B = dz[r].  The 16 transposed
// fragments of the 64 features nb are read by ce_read_yt — those of nb = 0 right in front of the product, or ahead of it
// (ce_rowpass_kernel) — and the product walks the blocks of 64, the next one's fragments requested in front of this one's MFMAs: 32
// fragment registers at any width, and every accumulator still adds its four rows in the order r = 0 .. 3
template <int EW>
__device__ __forceinline__ void ce_read_yt(float (&yt16)[4][4], const float* myY, int j, int g, int nb = 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int et = 0; et < 4; ++et) yt16[r][et] = myY[(4 * g + r) * (EW + 4) + 64 * nb + 16 * et + j];
}
template <int EW>
__device__ __forceinline__ void ce_second(f4 (&dacc)[EW / 16], float (&yt16)[4][4], const float (&dz)[4], const float* myY, int j, int g) {
#pragma unroll
    for (int nb = 0; nb < EW / 64; ++nb) {
        float nx[4][4];
        if (nb + 1 < EW / 64) ce_read_yt<EW>(nx, myY, j, g, nb + 1);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int et = 0; et < 4; ++et)
                dacc[4 * nb + et] = __builtin_amdgcn_mfma_f32_16x16x4f32(yt16[r][et], dz[r], dacc[4 * nb + et], 0, 0, 0);
        if (nb + 1 < EW / 64) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int et = 0; et < 4; ++et) yt16[r][et] = nx[r][et];
        }
    }
}

// the wave's accumulators into its plane of sRed, and (behind a barrier) the four planes summed into dX
template <int EW>
__device__ __forceinline__ void ce_dacc_to_red(CeRed<EW>& sRed, const f4 (&dacc)[EW / 16], int wave, int j, int g) {
#pragma unroll
    for (int et = 0; et < EW / 16; ++et)
#pragma unroll
        for (int r = 0; r < 4; ++r) sRed[wave][j][16 * et + 4 * g + r] = dacc[et][r];
}
template <int EW, class I>
__device__ __forceinline__ void ce_sum_store(const CeRed<EW>& sRed, float* __restrict__ dX, I x0, I NX, int tid) {
    for (int i = tid; i < 16 * EW; i += 256) {
        const int rj = i / EW, e = i - rj * EW;
        if (x0 + rj < NX) dX[(int64_t)(x0 + rj) * EW + e] = sRed[0][rj][e] + sRed[1][rj][e] + sRed[2][rj][e] + sRed[3][rj][e];
    }
}

// FWD, per tile: the lane's four logits folded into its running (max, sum).  One rescale per tile instead of a data-dependent branch
// with an exp on both sides per logit (5 exps per 4 logits instead of 8, no divergence); masked logits are finite (MASKV), structural
// padding is -inf -> 0.  EXP: expf in the plain kernel, fexp in the row pass
template <class EXP>
__device__ __forceinline__ void ce_online(float& run_m, float& run_l, const float (&fv)[4], EXP ex) {
    const float m4 = fmaxf(fmaxf(fv[0], fv[1]), fmaxf(fv[2], fv[3]));
    const float mn = fmaxf(run_m, m4);
    if (mn > -INFINITY) {
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) add += ex(fv[r] - mn);
        run_l = run_l * ex(run_m - mn) + add;
        run_m = mn;
    }
}

// FWD, after the walk: (m, l) and the label logit combined across the 4 lane groups and the 4 waves; lse and the row loss of X row x
template <int EW, class I>
__device__ __forceinline__ void ce_fwd_finish(CeRed<EW>& sRed, float run_m, float run_l, float zlab, int wave, int j, int g, bool xok, I x,
                                              bool row_valid, const CeBufs& b) {
    auto comb = [](float& m, float& l, float m2, float l2) {
        const float mn = fmaxf(m, m2);
        const float a = m == -INFINITY ? 0.f : l * expf(m - mn);
        const float c = m2 == -INFINITY ? 0.f : l2 * expf(m2 - mn);
        m = mn;
        l = a + c;
    };
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
        const float m2 = __shfl_xor(run_m, o, 64), l2 = __shfl_xor(run_l, o, 64);
        comb(run_m, run_l, m2, l2);
        zlab += __shfl_xor(zlab, o, 64);
    }
    if (g == 0) {
        sRed[wave][j][0] = run_m;
        sRed[wave][j][1] = run_l;
        sRed[wave][j][2] = zlab;
    }
    __syncthreads();
    if (wave == 0 && g == 0 && xok) {
        float m = sRed[0][j][0], l = sRed[0][j][1], zl = sRed[0][j][2];
        for (int w = 1; w < 4; ++w) {
            comb(m, l, sRed[w][j][0], sRed[w][j][1]);
            zl += sRed[w][j][2];
        }
        const float lse = m + logf(l);
        b.lse[x] = lse;
        b.rowloss[x] = row_valid ? lse - zl : 0.f;
    }
}

// The finish of the fused forward + d_prec passes (ce_rowpass_kernel<CE_FUSED>: its four waves, from LDS; ce16_row_combine_kernel: the
// Y ranges of the split route, from the workspace), for feature e of prec row xr.  part(w, k) is partial result w = 0 .. n - 1 of the
// row: k < EW the accumulator sum_y exp(z - m_w) score[y][k], k = EW its maximum m_w, EW + 1 its sum l_w, EW + 2 its label logit.  The
// partials are brought to the common maximum in the order w = 0, 1, ...;  d_prec = (sum_y p_y score_y - score_label) / n for d_loss = 1.
// labv(lab) is score[lab][e] AS THE PASS'S PRODUCTS SAW IT (the f32 value, or hi + lo of the split planes): where p_label = 1 the two
// terms then cancel to the bit.  A label column that is history padding keeps its fill value (model.py:88-89 assigns it): no gradient
template <int EW, class PART, class LABV>
__device__ __forceinline__ void ce_fused_finish(int n, PART part, LABV labv, int xr, int e,
                                                const float* __restrict__ log_mask, const CeBufs& b, int S) {
#pragma clang fp contract(off)      // the two sums below as written (l fused, acc not), whatever else the caller inlines around them
    float m = part(0, EW);
    for (int w = 1; w < n; ++w) m = fmaxf(m, part(w, EW));
    float l = 0.f, acc = 0.f, zl = 0.f;
    for (int w = 0; w < n; ++w) {
        const float f = fexp(part(w, EW) - m);
        l = fmaf(part(w, EW + 1), f, l);
        acc += part(w, e) * f;
        zl += part(w, EW + 2);
    }
    const bool valid = log_mask[xr] != 0.f;
    const int lab = ce_label(xr, S);
    b.dprec[(int64_t)xr * EW + e] = valid ? (acc / l - (b.colpad[lab] ? 0.f : labv(lab))) / b.nvalid[0] : 0.f;
    if (e == 0) {
        const float lse = m + logf(l);
        b.lse[xr] = lse;
        b.rowloss[xr] = valid ? lse - zl : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The plain kernel: the loss as it is defined, one logit at a time.  X rows: prec (FWD, DPREC) or score (DSCORE); Y rows: the other
// matrix.  Every logit (row, col) fetches its own column id / padding flag / debias, its row's lse and mask, and scans the row's
// sequence for the id (id_in_seq) — 3 + S1 loads per logit, 64-bit indices, libm expf: 2.9 ms forward + backward at bs = 1024, S = 10
// against 0.85 ms of the row-fixed passes (profiles/ce_shared_core.md).  It serves the shapes the row-fixed kernels do not take
// (S < 5, S > 15, M >= 2^31) and is the text they are read against.
template <int MODE, int EW>
__global__ __launch_bounds__(256) void ce_pass_kernel(const float* __restrict__ prec, const float* __restrict__ score,
                                                      const float* __restrict__ log_mask, CeBufs b, int64_t bs, int S,
                                                      float d_loss, float* __restrict__ dX) {
    static_assert(MODE == CE_FWD || MODE == CE_DPREC || MODE == CE_DSCORE, "the fused forward exists in the row-fixed kernels only");
    __shared__ __attribute__((aligned(16))) float sY[4][16 * (EW + 4)];
    __shared__ CeRedOwn<EW> sRedOwn;
    CeRed<EW>& sRed = ce_red<EW>(sY, sRedOwn);
    const int S1 = S + 1;
    const int64_t T = bs * S, M = bs * S1;
    const float* X = MODE == CE_DSCORE ? score : prec;
    const float* Y = MODE == CE_DSCORE ? prec : score;
    const int64_t NX = MODE == CE_DSCORE ? M : T, NY = MODE == CE_DSCORE ? T : M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int64_t x0 = (int64_t)blockIdx.x * 16;
    const int64_t x = x0 + j;
    const bool xok = x < NX;
    const int64_t xc = xok ? x : NX - 1;
    float xb[EW / 4];
    ce_load_x<EW>(xb, X, xc, g);

    float run_m = -INFINITY, run_l = 0.f, zlab = 0.f;
    f4 dacc[EW / 16];
#pragma unroll
    for (int et = 0; et < EW / 16; ++et) dacc[et] = (f4){0.f, 0.f, 0.f, 0.f};
    float* myY = sY[wave];
    const int64_t ntiles = (NY + 15) / 16;
    for (int64_t yt = wave; yt < ntiles; yt += 4) {
        const int64_t y0 = yt * 16;
        f4 yreg[EW / 16];
        const int64_t yr = y0 + (lane >> 2);
#pragma unroll
        for (int nb = 0; nb < EW / 64; ++nb)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                yreg[4 * nb + v] = (f4){0.f, 0.f, 0.f, 0.f};
                if (yr < NY) yreg[4 * nb + v] = *(const f4*)ce_ypart<EW>(Y, yr, lane, nb, v);
            }
        ce_stage_y<EW>(myY, yreg, lane);
        __builtin_amdgcn_wave_barrier();
        const f4 z = ce_logits<EW>(myY, xb, j, g);
        float dz[4], fv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t y = y0 + 4 * g + r;
            const bool yok = y < NY;
            const int64_t yc = yok ? y : NY - 1;
            const int64_t row = MODE == CE_DSCORE ? yc : xc, col = MODE == CE_DSCORE ? xc : yc;
            const int64_t label = ce_label(row, S);
            float val = z[r] - b.debias[col];
            if (b.colpad[col]) val = MASKV;
            else if (col != label && id_in_seq(b.ids32, row / S, S1, b.ids32[col])) val = MASKV;
            if (MODE == CE_FWD) {
                fv[r] = yok ? val : -INFINITY;
                if (yok && col == label) zlab = val;
            } else {
                const float scale = log_mask[row] != 0.f ? d_loss / b.nvalid[0] : 0.f;
                const float p = expf(val - b.lse[row]);
                dz[r] = (yok && xok) ? (p - ((col == label && !b.colpad[col]) ? 1.f : 0.f)) * scale : 0.f;
            }
        }
        if (MODE == CE_FWD) {
            ce_online(run_m, run_l, fv, [](float v) { return expf(v); });
        } else {
            float yt16[4][4];
            ce_read_yt<EW>(yt16, myY, j, g);
            ce_second<EW>(dacc, yt16, dz, myY, j, g);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (MODE == CE_FWD) {
        ce_fwd_finish<EW>(sRed, run_m, run_l, zlab, wave, j, g, xok, x, xok && log_mask[xc] != 0.f, b);
    } else {
        ce_dacc_to_red<EW>(sRed, dacc, wave, j, g);
        __syncthreads();
        ce_sum_store<EW>(sRed, dX, x0, NX, tid);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The row-fixed passes (X = prec, Y = score; FWD, DPREC, and FUSED = both in one walk) with the per-logit work cut down.  rocprofv3 of
// the Cached step at bs = 1024 had the plain passes at 476 / 586 / 634 us against 110 / 220 / 220 us of f32 MFMA time: they were
// VALU-bound (~100 VALU instructions per logit).  What is particular here:
//   * the false-negative test is done ONCE PER WAVE AND TILE: the 16 rows of a workgroup belong to at most four sequences
//     (S >= 5), lane l tests column l&15 against the ids of sequence slot l>>4 (held in its registers for the whole pass, RS1 of
//     them: 11 = the reference's max_seq_len 10 + 1, or MAXS1) and a ballot turns the 64 answers into a mask every lane indexes
//     with (its row's slot, the logit's column);
//   * column padding is a second ballot, the debias of a lane's four columns one 16-byte LDS read;
//   * fexp instead of expf, 32-bit indices;
//   * the next tile's rows and column metadata travel in registers while the current tile is multiplied, and the second product's
//     fragments are read ahead of the mask / exp arithmetic.
// CE_FUSED: forward and d_prec in ONE pass, flash-attention style: the accumulators hold sum_y exp(z - run_m) * score[y] against a
// running ROW maximum (common to the four lanes of a row, because the MFMA sums over their columns) and are rescaled when it moves —
// after the first tiles it almost never does, and the test is one ballot per tile.  d_prec for d_loss = 1 stays in the workspace.
template <int MODE, int RS1, int EW>
__global__ __launch_bounds__(256) void ce_rowpass_kernel(const float* __restrict__ prec, const float* __restrict__ score,
                                                         const float* __restrict__ log_mask, CeBufs b, int bs, int S,
                                                         float d_loss, float* __restrict__ dX) {
    static_assert(MODE == CE_FWD || MODE == CE_DPREC || MODE == CE_FUSED, "row-fixed passes only");
    __shared__ __attribute__((aligned(16))) float sY[4][16 * (EW + 4)];
    __shared__ CeRedOwn<EW> sRedOwn;
    CeRed<EW>& sRed = ce_red<EW>(sY, sRedOwn);
    __shared__ __attribute__((aligned(16))) int sMeta[4][64];    // per wave: ids | pad flags | debias of the tile's 16 columns
    const int S1 = S + 1;
    const int T = bs * S, M = bs * S1;
    const float* X = prec;
    const float* Y = score;
    const int NX = T, NY = M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * 16;
    const int x = x0 + j;
    const bool xok = x < NX;
    const int xc = xok ? x : NX - 1;

    float xb[EW / 4];
    ce_load_x<EW>(xb, X, xc, g);
    const int row_seq = xc / S;
    const int row_label = ce_label(xc, S);
    const bool row_valid = xok && log_mask[xc] != 0.f;
    const float row_lse = MODE == CE_DPREC ? b.lse[xc] : 0.f;
    const float row_scale = (MODE == CE_DPREC && row_valid) ? d_loss / b.nvalid[0] : 0.f;
    const int seq0 = x0 / S;
    const int row_shift = (row_seq - seq0) * 16 + 4 * g;       // bit of (my row's slot, column 4g) in the tile's hit mask
    // ids of sequence slot g = lane>>4 of this workgroup, for the cooperative false-negative test
    int sid[RS1];
    {
        const int sq = seq0 + g;
#pragma unroll
        for (int p = 0; p < RS1; ++p) sid[p] = (p < S1 && sq < bs) ? b.ids32[sq * S1 + p] : -2;
    }

    float run_m = MODE == CE_FUSED ? -3.0e38f : -INFINITY, run_l = 0.f, zlab = 0.f;
    f4 dacc[EW / 16];
#pragma unroll
    for (int et = 0; et < EW / 16; ++et) dacc[et] = (f4){0.f, 0.f, 0.f, 0.f};

    float* myY = sY[wave];
    int* myMeta = sMeta[wave];
    const int ntiles = (NY + 15) / 16;
    // the prefetch registers: with the loads at the top of the iteration every tile waited for an L2 round trip (FWD 303 us against
    // 110 us of MFMA time)
    f4 yreg[EW / 16];
    int mreg[3] = {0, 0, 0};
    // Branch-free: a tile index past the end re-reads the last tile, a row past NY re-reads row NY-1 (finite values that
    // meet dz = 0) — every conditional load was a saveexec / branch pair in the loop, and a join makes the waitcnt pass drain.
    auto prefetch = [&](int yt_) {
        const int y0_ = (yt_ < ntiles ? yt_ : ntiles - 1) * 16;
        const int r = lane >> 2, ch = lane & 3;
        const int yr = y0_ + r < NY ? y0_ + r : NY - 1;
        const float* yp = Y + (int64_t)yr * EW + ch * 16;
#pragma unroll
        for (int nb = 0; nb < EW / 64; ++nb)
#pragma unroll
            for (int v = 0; v < 4; ++v) yreg[4 * nb + v] = *(const f4*)(yp + 64 * nb + v * 4);
        const int cc = y0_ + (lane & 15) < NY ? y0_ + (lane & 15) : NY - 1;
        mreg[0] = b.ids32[cc];
        mreg[1] = b.colpad[cc];
        mreg[2] = __float_as_int(b.debias[cc]);
    };
    prefetch(wave);
    for (int yt = wave; yt < ntiles; yt += 4) {
        const int y0 = yt * 16;
        ce_stage_y<EW>(myY, yreg, lane);
        if (lane < 16) {
            myMeta[lane] = mreg[0];
            myMeta[16 + lane] = mreg[1];
            myMeta[32 + lane] = mreg[2];
        }
        prefetch(yt + 4);
        __builtin_amdgcn_wave_barrier();
        // once per wave and tile: (sequence slot g, column j) hit bits and the 16 column-padding bits
        const int idc = myMeta[j];
        bool h = false;
#pragma unroll
        for (int p = 0; p < RS1; ++p) h |= sid[p] == idc;
        const unsigned long long hm = __ballot(h);
        const unsigned pm = (unsigned)__ballot(myMeta[16 + j] != 0);
        const unsigned hit4 = (unsigned)(hm >> row_shift) & 0xfu;
        const unsigned pad4 = (pm >> (4 * g)) & 0xfu;
        const f4 deb4 = *(const f4*)(myMeta + 32 + 4 * g);      // bit patterns of four floats

        const f4 z = ce_logits<EW>(myY, xb, j, g);
        // the second product's 16 transposed tile reads (of its first 64 features) are requested NOW, fenced, and land behind the mask / exp arithmetic:
        // left to the compiler each pair sat right in front of its two MFMAs behind an lgkmcnt(0) (eight exposed LDS
        // round trips per tile)
        float yt16[4][4];
        if (MODE != CE_FWD) {
            ce_read_yt<EW>(yt16, myY, j, g);
            __builtin_amdgcn_sched_barrier(0);
        }
        const bool whole = y0 + 16 <= NY;            // wave-uniform
        const int lab_r = row_label - (y0 + 4 * g);  // r with column == label, if in 0..3
        float dz[4], fv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool is_lab = lab_r == r;
            const bool masked = ((pad4 >> r) & 1u) | (((hit4 >> r) & 1u) & (is_lab ? 0u : 1u));
            const float val = masked ? MASKV : z[r] - deb4[r];
            const bool yok = whole || (y0 + 4 * g + r < NY);
            if (MODE == CE_FWD || MODE == CE_FUSED) {
                fv[r] = yok ? val : -INFINITY;
                if (yok && is_lab) zlab = val;
            } else {
                const float pr = fexp(val - row_lse);
                dz[r] = (yok && xok) ? (pr - ((is_lab && !((pad4 >> r) & 1u)) ? 1.f : 0.f)) * row_scale : 0.f;
            }
        }
        if (MODE == CE_FWD) {
            ce_online(run_m, run_l, fv, fexp);
        } else {
            if (MODE == CE_FUSED) {
                const float m4 = fmaxf(fmaxf(fv[0], fv[1]), fmaxf(fv[2], fv[3]));
                if (__ballot(m4 > run_m)) {              // wave-uniform and rare
                    float mr = fmaxf(m4, __shfl_xor(m4, 16, 64));
                    mr = fmaxf(mr, __shfl_xor(mr, 32, 64));
                    const float mn = fmaxf(run_m, mr);
                    const float f = fexp(run_m - mn);    // run_m starts at -3e38: f = 0 on the first tile
                    run_l *= f;
#pragma unroll
                    for (int et = 0; et < EW / 16; ++et) dacc[et] *= f;
                    run_m = mn;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    dz[r] = fexp(fv[r] - run_m);         // structural padding: exp(-inf) = 0
                    run_l += dz[r];
                }
            }
            ce_second<EW>(dacc, yt16, dz, myY, j, g);
        }
        __builtin_amdgcn_wave_barrier();
    }

    if (MODE == CE_FWD) {
        ce_fwd_finish<EW>(sRed, run_m, run_l, zlab, wave, j, g, xok, x, row_valid, b);
    } else if (MODE == CE_FUSED) {
        // the four lanes of a row share run_m; their sums add up
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            run_l += __shfl_xor(run_l, o, 64);
            zlab += __shfl_xor(zlab, o, 64);
        }
        ce_dacc_to_red<EW>(sRed, dacc, wave, j, g);
        if (g == 0) {
            sRed[wave][j][EW] = run_m;
            sRed[wave][j][EW + 1] = run_l;
            sRed[wave][j][EW + 2] = zlab;
        }
        __syncthreads();
        for (int i = tid; i < 16 * EW; i += 256) {
            const int rj = i / EW, e = i - rj * EW;
            const int xr = x0 + rj;
            if (xr >= NX) continue;
            ce_fused_finish<EW>(4, [&](int w, int k) { return sRed[w][rj][k]; }, [&](int lab) { return Y[(int64_t)lab * EW + e]; }, xr, e, log_mask, b, S);
        }
    } else {
        ce_dacc_to_red<EW>(sRed, dacc, wave, j, g);
        __syncthreads();
        ce_sum_store<EW>(sRed, dX, x0, NX, tid);
    }
}

__global__ void ce_scale_kernel(const float* __restrict__ in, float scale, float* __restrict__ out, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        f4 v = ((const f4*)in)[i];
        v *= scale;
        ((f4*)out)[i] = v;
    }
}

// The column-fixed pass (d_score = dZ^T · prec: X = score, Y = prec) in the same style: lane (j, g) owns column x0 + j for the whole
// pass and, per tile of 16 prec rows (at most four sequences), tests ITS column against the ids of the tile's sequence slot g — the
// four lanes of a column cover the four slots — and a ballot publishes the 64 answers; per-row label / lse / scale / slot come from
// a small LDS table, one 16-byte read each.  The tile's ids and per-row values are prefetched with its rows.
template <int RS1, int EW>
__global__ __launch_bounds__(256) void ce_colpass_kernel(const float* __restrict__ prec, const float* __restrict__ score,
                                                         const float* __restrict__ log_mask, CeBufs b, int bs, int S,
                                                         float d_loss, float* __restrict__ dX) {
    __shared__ __attribute__((aligned(16))) float sY[4][16 * (EW + 4)];
    __shared__ CeRedOwn<EW> sRedOwn;
    CeRed<EW>& sRed = ce_red<EW>(sY, sRedOwn);
    __shared__ __attribute__((aligned(16))) int sMeta[4][64];     // ids of the tile's four sequences, 16 per slot
    __shared__ __attribute__((aligned(16))) int sRow[4][64];      // per row: slot | label column | lse | scale
    const int S1 = S + 1;
    const int T = bs * S, M = bs * S1;
    const float* X = score;
    const float* Y = prec;
    const int NX = M, NY = T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int x0 = blockIdx.x * 16;
    const int x = x0 + j;
    const bool xok = x < NX;
    const int xc = xok ? x : NX - 1;

    float xb[EW / 4];
    ce_load_x<EW>(xb, X, xc, g);
    const int col_id = b.ids32[xc];
    const bool col_pad = b.colpad[xc] != 0;
    const float col_debias = b.debias[xc];
    const float dscale = d_loss / b.nvalid[0];

    f4 dacc[EW / 16];
#pragma unroll
    for (int et = 0; et < EW / 16; ++et) dacc[et] = (f4){0.f, 0.f, 0.f, 0.f};
    float* myY = sY[wave];
    int* myMeta = sMeta[wave];
    int* myRow = sRow[wave];
    const int ntiles = (NY + 15) / 16;
    f4 yreg[EW / 16];
    int idreg = -2;
    float lsereg = 0.f, lmreg = 0.f;
    auto prefetch = [&](int yt_) {
        const int y0_ = yt_ * 16;
        const int r = lane >> 2, ch = lane & 3;
        const int yr = y0_ + r;
#pragma unroll
        for (int nb = 0; nb < EW / 64; ++nb)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                yreg[4 * nb + v] = (f4){0.f, 0.f, 0.f, 0.f};
                if (yt_ < ntiles && yr < NY) yreg[4 * nb + v] = *(const f4*)(Y + (int64_t)yr * EW + 64 * nb + ch * 16 + v * 4);
            }
        if (yt_ < ntiles) {
            const int sq = y0_ / S + g;                 // lane (g, j): id j of the tile's sequence slot g
            idreg = (j < S1 && sq < bs) ? b.ids32[sq * S1 + j] : -2;
            if (lane < 16) {
                const int rw = y0_ + lane < NY ? y0_ + lane : NY - 1;
                lsereg = b.lse[rw];
                lmreg = log_mask[rw];
            }
        }
    };
    prefetch(wave);
    for (int yt = wave; yt < ntiles; yt += 4) {
        const int y0 = yt * 16;
        ce_stage_y<EW>(myY, yreg, lane);
        myMeta[lane] = idreg;
        if (lane < 16) {
            const int seq0 = y0 / S;
            const int rw = y0 + lane < NY ? y0 + lane : NY - 1;
            myRow[lane] = rw / S - seq0;
            myRow[16 + lane] = ce_label(rw, S);
            myRow[32 + lane] = __float_as_int(lsereg);
            myRow[48 + lane] = __float_as_int(lmreg != 0.f ? dscale : 0.f);
        }
        prefetch(yt + 4);
        __builtin_amdgcn_wave_barrier();
        typedef int i4 __attribute__((ext_vector_type(4)));
        bool h = false;
#pragma unroll
        for (int q = 0; q < (RS1 + 3) / 4; ++q) {
            const i4 v = *(const i4*)(myMeta + 16 * g + 4 * q);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * q + k < RS1) h |= v[k] == col_id;
        }
        const unsigned long long hm = __ballot(h);      // bit 16*slot + j
        const i4 slot4 = *(const i4*)(myRow + 4 * g);
        const i4 lab4 = *(const i4*)(myRow + 16 + 4 * g);
        const f4 lse4 = *(const f4*)(myRow + 32 + 4 * g);
        const f4 sc4 = *(const f4*)(myRow + 48 + 4 * g);

        const f4 z = ce_logits<EW>(myY, xb, j, g);
        const bool whole = y0 + 16 <= NY;
        float dz[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool is_lab = lab4[r] == xc;
            const bool hit = (hm >> (16 * slot4[r] + j)) & 1ull;
            const bool masked = col_pad | (hit & !is_lab);
            const float val = masked ? MASKV : z[r] - col_debias;
            const bool yok = whole || (y0 + 4 * g + r < NY);
            const float pr = fexp(val - lse4[r]);
            dz[r] = (yok && xok) ? (pr - ((is_lab && !col_pad) ? 1.f : 0.f)) * sc4[r] : 0.f;
        }
        float yt16[4][4];
        ce_read_yt<EW>(yt16, myY, j, g);
        ce_second<EW>(dacc, yt16, dz, myY, j, g);
        __builtin_amdgcn_wave_barrier();
    }
    ce_dacc_to_red<EW>(sRed, dacc, wave, j, g);
    __syncthreads();
    ce_sum_store<EW>(sRed, dX, x0, NX, tid);
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 6: the same two passes on the 16-bit matrix cores with SPLIT operands (the idea of split.hip, inside the loss).
// At the Cached batch size (bs = 1024: 10,240 x 11,264 logits) the f32-input passes above take 415 + 425 us per step against
// 2 x 220 us of v_mfma_f32_16x16x4_f32 time: 59 GFLOP on a 157 TF pipe.  Here prec and score are split once per call into
// fp16 planes, x s = hi + lo (s a power of two from the tensor's amax), and
//     logits      = (Xh Yh^T + Xh Yl^T + Xl Yh^T) / (sx sy)            3 x v_mfma_f32_16x16x32_f16 per 16 x 16 x 32 block
//     dX^T       += (Yh^T Qh + Yh^T Ql + Yl^T Qh) / (sy 2^10)          Q = the exp / probability registers, split the same way
// — a 16 x 16 tile pair costs 12 + 12 sixteen-cycle MFMAs instead of 32 thirty-two-cycle ones, the passes become VALU-bound
// (mask, exp, split: ~25 instructions per logit).  Accuracy as split.hip: 22 mantissa bits of every element within 2^-16 of
// the tensor's amax, the dropped lo x lo term 2^-22 relative.
// Shape: a workgroup = 64 x NSUB X rows (a wave owns NSUB blocks of 16) x one of `ysplits` ranges of Y; every step stages 32 Y
// rows for all four waves — row-major (A operand of the logits) and transposed (A operand of the second product), hi and lo,
// four contiguous 4 KB blocks of the images ce16_split_kernel wrote — double-buffered, one barrier per step.  A wave keeps
// its rows' online-softmax state; the per-range partial results meet in a small combine kernel (fixed order: bit-reproducible).
// The 8 probabilities a lane holds after the two logit tiles of a step ARE the B operand of the second product (K-slot t of
// lane group g <-> Y row 4g + t | 16 + 4g + (t - 4) of the step: the transposed images are stored in that order).
constexpr int C16_YLD = 72;            // halves per LDS row of the row-major tile (128 B + 16: conflict-free ds_read_b128)
constexpr int C16_TLD = 40;            // halves per LDS row of the transposed tile (64 B + 16)
constexpr float C16_QS = 1024.f;       // the probability registers are split at this scale (they are <= 1 in magnitude)
constexpr int C16_MAX_YS = 16;

struct Ce16Bufs {
    uint32_t* amax;            // [2]: bit patterns of max|prec|, max|score|
    _Float16* img[2][2];       // [prec | score][hi | lo]: row-major [N padded to 32][64]
    _Float16* imgT[2][2];      // the same rows transposed per group of 32: [group][64][32 slots]
    float* part_row;           // [ysplits][T][68]: sum_y exp(z - m) score_y (64) | m | l | z_label | -
    float* part_col;           // [ysplits][M][64]
};

void carve16(WsCarver& c, Ce16Bufs& b, int64_t bs, int S) {
    const size_t M = (size_t)bs * (S + 1), T = (size_t)bs * S;
    const size_t n[2] = {align_up(T, 32), align_up(M, 32)};
    b.amax = c.take<uint32_t>(4);
    for (int t = 0; t < 2; ++t)
        for (int pl = 0; pl < 2; ++pl) {
            b.img[t][pl] = c.take<_Float16>(n[t] * E);
            b.imgT[t][pl] = c.take<_Float16>(n[t] * E);
        }
    b.part_row = c.take<float>((size_t)C16_MAX_YS * T * 68);
    b.part_col = c.take<float>((size_t)C16_MAX_YS * M * E);
}

__device__ __forceinline__ float c16_scale_of(uint32_t amax_bits) {       // as split.hip: the largest element lands in [2^13, 2^14)
    const int e = (int)(amax_bits >> 23) & 0xff;
    if (e == 0 || e == 0xff) return 1.0f;
    return __uint_as_float((uint32_t)(267 - e) << 23);
}

__global__ __launch_bounds__(256) void ce16_amax_kernel(const float* __restrict__ prec, int64_t n0, const float* __restrict__ score, int64_t n1,
                                                        uint32_t* amax) {
    __shared__ float red[4];
    const float* x = blockIdx.y ? score : prec;
    const int64_t n4 = (blockIdx.y ? n1 : n0) / 4;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const f4 v = ((const f4*)x)[i];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (m > 0.f) atomicMax(amax + blockIdx.y, __float_as_uint(m));
    }
}

// slot of Y row r (0..31) of a step inside the transposed image: lane group g = slot >> 3 holds rows 4g..4g+3 | 16+4g..16+4g+3
__device__ __forceinline__ int c16_slot(int r) { return r < 16 ? 8 * (r >> 2) + (r & 3) : 8 * ((r - 16) >> 2) + 4 + (r & 3); }

// one workgroup = 32 rows of one tensor (blockIdx.y): the four images of that group
__global__ __launch_bounds__(256) void ce16_split_kernel(const float* __restrict__ prec, int64_t T, const float* __restrict__ score, int64_t M, Ce16Bufs c) {
    __shared__ _Float16 sT[2][E][32 + 2];
    const int t = blockIdx.y;
    const float* x = t ? score : prec;
    const int64_t N = t ? M : T, groups = (N + 31) / 32;
    if ((int64_t)blockIdx.x >= groups) return;
    const float s = c16_scale_of(c.amax[t]);
    const int tid = threadIdx.x, r = tid >> 3, c8 = (tid & 7) * 8;
    const int64_t row = (int64_t)blockIdx.x * 32 + r;
    h8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) { hi[e] = (_Float16)0.f; lo[e] = (_Float16)0.f; }
    if (row < N) {
        const f4 v0 = *(const f4*)(x + row * E + c8), v1 = *(const f4*)(x + row * E + c8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = v0[e] * s, bq = v1[e] * s;
            hi[e] = (_Float16)a; lo[e] = (_Float16)(a - (float)hi[e]);
            hi[4 + e] = (_Float16)bq; lo[4 + e] = (_Float16)(bq - (float)hi[4 + e]);
        }
    }
    *(h8*)(c.img[t][0] + row * E + c8) = hi;
    *(h8*)(c.img[t][1] + row * E + c8) = lo;
    const int slot = c16_slot(r);
#pragma unroll
    for (int e = 0; e < 8; ++e) { sT[0][c8 + e][slot] = hi[e]; sT[1][c8 + e][slot] = lo[e]; }
    __syncthreads();
    const int er = tid >> 2, p8 = (tid & 3) * 8;
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        h8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = sT[pl][er][p8 + e];
        *(h8*)(c.imgT[t][pl] + ((int64_t)blockIdx.x * E + er) * 32 + p8) = v;
    }
}

// the staged tiles of one step, shared by the four waves
struct C16Tiles {
    _Float16 yh[32 * C16_YLD], yl[32 * C16_YLD], th[E * C16_TLD], tl[E * C16_TLD];
};
struct C16Stage {      // one thread's share of a step in flight: a 16-byte piece of each of the four tiles
    h8 yh, yl, th, tl;
};
__device__ __forceinline__ void c16_load(C16Stage& st, const Ce16Bufs& c, int ty, int64_t step, int tid) {
    const int64_t o = step * (32 * E) + tid * 8;
    st.yh = *(const h8*)(c.img[ty][0] + o);
    st.yl = *(const h8*)(c.img[ty][1] + o);
    st.th = *(const h8*)(c.imgT[ty][0] + o);
    st.tl = *(const h8*)(c.imgT[ty][1] + o);
}
__device__ __forceinline__ void c16_store(C16Tiles& t, const C16Stage& st, int tid) {
    const int yo = (tid >> 3) * C16_YLD + (tid & 7) * 8, to = (tid >> 2) * C16_TLD + (tid & 3) * 8;
    *(h8*)(t.yh + yo) = st.yh;
    *(h8*)(t.yl + yo) = st.yl;
    *(h8*)(t.th + to) = st.th;
    *(h8*)(t.tl + to) = st.tl;
}
// logits^T of one half (16 Y rows) of the step against the 16 X rows whose fragments the lane holds: lane (j, g) -> X row j, Y rows 4g..4g+3.
// The three terms are added in the order score_hi prec_hi, score_hi prec_lo, score_lo prec_hi in BOTH passes (COL: Y = prec), so the column
// pass sees the logits of the row pass's lse to the bit: where a row's probability is all on its label, p - 1 is exactly 0
template <bool COL>
__device__ __forceinline__ f4 c16_logits(const C16Tiles& t, int half, int j, int g, const h8 (&xh)[2], const h8 (&xl)[2]) {
    f4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
        const int o = (16 * half + j) * C16_YLD + 32 * cc + 8 * g;
        const h8 ah = *(const h8*)(t.yh + o), al = *(const h8*)(t.yl + o);
        z = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, xh[cc], z, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f32_16x16x32_f16(COL ? al : ah, COL ? xh[cc] : xl[cc], z, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f32_16x16x32_f16(COL ? ah : al, COL ? xl[cc] : xh[cc], z, 0, 0, 0);
    }
    return z;
}
// dacc[et] += Y^T (16 features of block et x the step's 32 rows) · Q (32 rows x the lane's X row), Q split at C16_QS
__device__ __forceinline__ void c16_second(const C16Tiles& t, int j, int g, const float (&q)[8], f4 (&dacc)[4]) {
    h8 bh, bl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = q[e] * C16_QS;
        bh[e] = (_Float16)v;
        bl[e] = (_Float16)(v - (float)bh[e]);
    }
    // fragments one feature block ahead, fenced: left alone the compiler requests all eight up front (32 registers that cost the pass a wave of occupancy)
    const int o0 = j * C16_TLD + 8 * g;
    h8 ah = *(const h8*)(t.th + o0), al = *(const h8*)(t.tl + o0);
#pragma unroll
    for (int et = 0; et < 4; ++et) {
        h8 nh = ah, nl = al;
        if (et < 3) {
            nh = *(const h8*)(t.th + o0 + 16 * (et + 1) * C16_TLD);
            nl = *(const h8*)(t.tl + o0 + 16 * (et + 1) * C16_TLD);
        }
        __builtin_amdgcn_sched_barrier(0);
        dacc[et] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, dacc[et], 0, 0, 0);
        dacc[et] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, dacc[et], 0, 0, 0);
        dacc[et] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, dacc[et], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        ah = nh; al = nl;
    }
}

// Fused forward + d_prec row pass (the online softmax of ce_rowpass_kernel<CE_FUSED>): X = prec, Y = score.  grid (x blocks, ysplits)
template <int RS1, int NSUB>
__global__ __launch_bounds__(256, NSUB == 1 ? 4 : 2) void ce16_rowpass_kernel(const float* __restrict__ log_mask, CeBufs b, Ce16Bufs c, int bs, int S, int steps_per) {
    __shared__ __attribute__((aligned(16))) C16Tiles tiles[2];
    __shared__ __attribute__((aligned(16))) int sMeta[2][96];          // per step: ids[32] | padding[32] | debias[32]
    __shared__ __attribute__((aligned(16))) int sSid[4][NSUB][64];     // per wave and X block: the ids of its four sequence slots, 16 per slot
    const int S1 = S + 1;
    const int T = bs * S, M = bs * S1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const float inv_z = 1.0f / (c16_scale_of(c.amax[0]) * c16_scale_of(c.amax[1]));
    const float inv_d = 1.0f / (c16_scale_of(c.amax[1]) * C16_QS);
    h8 xh[NSUB][2], xl[NSUB][2];
    int row_label[NSUB], row_shift[NSUB];
    bool xok[NSUB];
    int xrow[NSUB];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
        const int x0 = (blockIdx.x * NSUB + u) * 64 + wave * 16;
        const int x = x0 + j;
        xok[u] = x < T;
        xrow[u] = x;
        const int xc = xok[u] ? x : T - 1;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            xh[u][cc] = *(const h8*)(c.img[0][0] + (int64_t)xc * E + 32 * cc + 8 * g);
            xl[u][cc] = *(const h8*)(c.img[0][1] + (int64_t)xc * E + 32 * cc + 8 * g);
        }
        const int row_seq = xc / S, seq0 = x0 / S;
        row_label[u] = row_seq * S1 + (xc - row_seq * S) + 1;
        row_shift[u] = xok[u] ? (row_seq - seq0) * 16 + 4 * g : 4 * g;
        const int sq = seq0 + g;
        sSid[wave][u][lane] = (j < S1 && sq < bs) ? b.ids32[sq * S1 + j] : -2;      // (read back by the same wave only; the first barrier below orders it)
    }
    float run_m[NSUB], run_l[NSUB], zlab[NSUB];
    f4 dacc[NSUB][4];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
        run_m[u] = -3.0e38f; run_l[u] = 0.f; zlab[u] = 0.f;
#pragma unroll
        for (int et = 0; et < 4; ++et) dacc[u][et] = (f4){0.f, 0.f, 0.f, 0.f};
    }
    const int steps_total = (M + 31) / 32;
    const int st0 = blockIdx.y * steps_per;
    int st1 = st0 + steps_per;
    if (st1 > steps_total) st1 = steps_total;
    C16Stage stg;
    int mreg[3] = {0, 0, 0};
    auto fetch = [&](int st) {
        st = st < st1 ? st : st1 - 1;                                   // past the end: the last step again (never used)
        c16_load(stg, c, 1, st, tid);
        if (tid < 32) {
            const int y = st * 32 + tid < M ? st * 32 + tid : M - 1;
            mreg[0] = b.ids32[y];
            mreg[1] = b.colpad[y];
            mreg[2] = __float_as_int(b.debias[y]);
        }
    };
    auto put = [&](int buf) {
        c16_store(tiles[buf], stg, tid);
        if (tid < 32) { sMeta[buf][tid] = mreg[0]; sMeta[buf][32 + tid] = mreg[1]; sMeta[buf][64 + tid] = mreg[2]; }
    };
    if (st0 < st1) {
        fetch(st0);
        put(0);
        __syncthreads();
    }
    for (int st = st0; st < st1; ++st) {
        const int buf = (st - st0) & 1;
        fetch(st + 1);
        const C16Tiles& tl = tiles[buf];
        const int* meta = sMeta[buf];
        const int y0 = st * 32;
        const bool whole = y0 + 32 <= M;                                // block-uniform
#pragma unroll
        for (int u = 0; u < NSUB; ++u) {
            float fv[8];
            bool lab[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f4 z = c16_logits<false>(tl, h, j, g, xh[u], xl[u]);
                // once per wave and half: (sequence slot g, column j) hit bits and the 16 column-padding bits
                const int idc = meta[16 * h + j];
                bool hit = false;
                {
                    typedef int i4 __attribute__((ext_vector_type(4)));
#pragma unroll
                    for (int qq = 0; qq < (RS1 + 3) / 4; ++qq) {
                        const i4 v = *(const i4*)(sSid[wave][u] + 16 * g + 4 * qq);
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (4 * qq + k < RS1) hit |= v[k] == idc;
                    }
                }
                const unsigned long long hm = __ballot(hit);
                const unsigned pm = (unsigned)__ballot(meta[32 + 16 * h + j] != 0);
                const unsigned hit4 = (unsigned)(hm >> row_shift[u]) & 0xfu;
                const unsigned pad4 = (pm >> (4 * g)) & 0xfu;
                const f4 deb4 = *(const f4*)(meta + 64 + 16 * h + 4 * g);
                const int lab_r = row_label[u] - (y0 + 16 * h + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool is_lab = lab_r == r;
                    const bool masked = ((pad4 >> r) & 1u) | (((hit4 >> r) & 1u) & (is_lab ? 0u : 1u));
                    const float val = masked ? MASKV : z[r] * inv_z - deb4[r];
                    const bool yok = whole || (y0 + 16 * h + 4 * g + r < M);
                    fv[4 * h + r] = yok ? val : -INFINITY;
                    lab[4 * h + r] = yok && is_lab;
                }
            }
            float m8 = fv[0];
#pragma unroll
            for (int e = 1; e < 8; ++e) m8 = fmaxf(m8, fv[e]);
            if (__ballot(m8 > run_m[u])) {                               // wave-uniform and rare after the first steps
                float mr = fmaxf(m8, __shfl_xor(m8, 16, 64));
                mr = fmaxf(mr, __shfl_xor(mr, 32, 64));
                const float mn = fmaxf(run_m[u], mr);
                const float f = fexp(run_m[u] - mn);                     // run_m starts at -3e38: f = 0 on the first step
                run_l[u] *= f;
#pragma unroll
                for (int et = 0; et < 4; ++et) dacc[u][et] *= f;
                run_m[u] = mn;
            }
            float q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                q[e] = fexp(fv[e] - run_m[u]);                           // structural padding: exp(-inf) = 0
                run_l[u] += q[e];
                if (lab[e]) zlab[u] = fv[e];
            }
            c16_second(tl, j, g, q, dacc[u]);
        }
        put(buf ^ 1);
        __syncthreads();
    }
    // per-range partial results of the wave's rows (the four lanes of a row share run_m; their sums add up)
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            run_l[u] += __shfl_xor(run_l[u], o, 64);
            zlab[u] += __shfl_xor(zlab[u], o, 64);
        }
        if (!xok[u]) continue;
        float* out = c.part_row + ((int64_t)blockIdx.y * T + xrow[u]) * 68;
#pragma unroll
        for (int et = 0; et < 4; ++et) *(f4*)(out + 16 * et + 4 * g) = dacc[u][et] * inv_d;
        if (g == 0) *(f4*)(out + E) = (f4){run_m[u], run_l[u], zlab[u], 0.f};
    }
}

// lse, row loss and d_prec (for d_loss = 1) from the per-range partial results: the ranges brought to the common maximum, fixed order
__global__ __launch_bounds__(256) void ce16_row_combine_kernel(const float* __restrict__ log_mask, CeBufs b, Ce16Bufs c,
                                                               int bs, int S, int ysplits) {
    const int T = bs * S;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int xr = i >> 6, e = i & 63;
    if (xr >= T) return;
    const float inv_s = 1.0f / c16_scale_of(c.amax[1]);
    ce_fused_finish<E>(ysplits, [&](int y, int k) { return c.part_row[((int64_t)y * T + xr) * 68 + k]; },
                    [&](int lab) { return ((float)c.img[1][0][(int64_t)lab * E + e] + (float)c.img[1][1][(int64_t)lab * E + e]) * inv_s; },
                    xr, e, log_mask, b, S);
}

// The column-fixed pass (d_score = dZ^T · prec): X = score (a lane owns one column), Y = prec.  grid (x blocks, ysplits)
template <int RS1, int NSUB>
__global__ __launch_bounds__(256, NSUB == 1 ? 4 : 2) void ce16_colpass_kernel(const float* __restrict__ log_mask, CeBufs b, Ce16Bufs c, int bs, int S, int steps_per) {
    __shared__ __attribute__((aligned(16))) C16Tiles tiles[2];
    __shared__ __attribute__((aligned(16))) int sIds[2][128];          // per half: ids of its four sequence slots, 16 per slot
    __shared__ __attribute__((aligned(16))) int sRow[2][4][32];        // per Y row: slot within its half | label column | lse | valid
    const int S1 = S + 1;
    const int T = bs * S, M = bs * S1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const float inv_z = 1.0f / (c16_scale_of(c.amax[0]) * c16_scale_of(c.amax[1]));
    const float inv_d = 1.0f / (c16_scale_of(c.amax[0]) * C16_QS);
    h8 xh[NSUB][2], xl[NSUB][2];
    int col_id[NSUB], xcol[NSUB];
    bool col_pad[NSUB], xok[NSUB];
    float col_debias[NSUB];
    f4 dacc[NSUB][4];
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
        const int x = (blockIdx.x * NSUB + u) * 64 + wave * 16 + j;
        xok[u] = x < M;
        xcol[u] = x;
        const int xc = xok[u] ? x : M - 1;
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            xh[u][cc] = *(const h8*)(c.img[1][0] + (int64_t)xc * E + 32 * cc + 8 * g);
            xl[u][cc] = *(const h8*)(c.img[1][1] + (int64_t)xc * E + 32 * cc + 8 * g);
        }
        col_id[u] = b.ids32[xc];
        col_pad[u] = b.colpad[xc] != 0;
        col_debias[u] = b.debias[xc];
#pragma unroll
        for (int et = 0; et < 4; ++et) dacc[u][et] = (f4){0.f, 0.f, 0.f, 0.f};
    }
    const int steps_total = (T + 31) / 32;
    const int st0 = blockIdx.y * steps_per;
    int st1 = st0 + steps_per;
    if (st1 > steps_total) st1 = steps_total;
    C16Stage stg;
    int mreg[4] = {0, 0, 0, 0};
    auto fetch = [&](int st) {
        st = st < st1 ? st : st1 - 1;
        c16_load(stg, c, 0, st, tid);
        if (tid < 128) {                       // thread (half, slot, id index): id of the half's sequence slot
            const int h = tid >> 6, sl = (tid >> 4) & 3, k = tid & 15;
            const int sq = (st * 32 + 16 * h) / S + sl;
            mreg[0] = (k < S1 && sq < bs) ? b.ids32[sq * S1 + k] : -2;
        } else if (tid < 160) {                // one Y row each
            const int r = tid - 128, y = st * 32 + r;
            const int yc = y < T ? y : T - 1;
            const int rs = yc / S;
            const int sl = rs - (st * 32 + 16 * (r >> 4)) / S;          // 0..3 for real rows (S >= 5); rows past T never count
            mreg[0] = sl < 0 ? 0 : (sl > 3 ? 3 : sl);
            mreg[1] = rs * S1 + (yc - rs * S) + 1;
            mreg[2] = __float_as_int(b.lse[yc]);
            mreg[3] = __float_as_int((y < T && log_mask[yc] != 0.f) ? 1.f : 0.f);
        }
    };
    auto put = [&](int buf) {
        c16_store(tiles[buf], stg, tid);
        if (tid < 128) sIds[buf][tid] = mreg[0];
        else if (tid < 160) {
            const int r = tid - 128;
            sRow[buf][0][r] = mreg[0]; sRow[buf][1][r] = mreg[1]; sRow[buf][2][r] = mreg[2]; sRow[buf][3][r] = mreg[3];
        }
    };
    if (st0 < st1) {
        fetch(st0);
        put(0);
        __syncthreads();
    }
    typedef int i4 __attribute__((ext_vector_type(4)));
    for (int st = st0; st < st1; ++st) {
        const int buf = (st - st0) & 1;
        fetch(st + 1);
        const C16Tiles& tl = tiles[buf];
        const int y0 = st * 32;
        const bool whole = y0 + 32 <= T;
#pragma unroll
        for (int u = 0; u < NSUB; ++u) {
            float q[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f4 z = c16_logits<true>(tl, h, j, g, xh[u], xl[u]);
                bool hit = false;
#pragma unroll
                for (int qq = 0; qq < (RS1 + 3) / 4; ++qq) {
                    const i4 v = *(const i4*)(sIds[buf] + 64 * h + 16 * g + 4 * qq);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (4 * qq + k < RS1) hit |= v[k] == col_id[u];
                }
                const unsigned long long hm = __ballot(hit);            // bit 16 * slot + j
                const i4 slot4 = *(const i4*)(sRow[buf][0] + 16 * h + 4 * g);
                const i4 lab4 = *(const i4*)(sRow[buf][1] + 16 * h + 4 * g);
                const f4 lse4 = *(const f4*)(sRow[buf][2] + 16 * h + 4 * g);
                const f4 ok4 = *(const f4*)(sRow[buf][3] + 16 * h + 4 * g);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool is_lab = lab4[r] == xcol[u];
                    const bool hb = (hm >> (16 * slot4[r] + j)) & 1ull;
                    const bool masked = col_pad[u] | (hb & !is_lab);
                    const float val = masked ? MASKV : z[r] * inv_z - col_debias[u];
                    const bool yok = whole || (y0 + 16 * h + 4 * g + r < T);
                    const float pr = fexp(val - lse4[r]);
                    q[4 * h + r] = (yok && xok[u]) ? (pr - ((is_lab && !col_pad[u]) ? 1.f : 0.f)) * ok4[r] : 0.f;
                }
            }
            c16_second(tl, j, g, q, dacc[u]);
        }
        put(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < NSUB; ++u) {
        if (!xok[u]) continue;
        float* out = c.part_col + ((int64_t)blockIdx.y * M + xcol[u]) * E;
#pragma unroll
        for (int et = 0; et < 4; ++et) *(f4*)(out + 16 * et + 4 * g) = dacc[u][et] * inv_d;
    }
}

__global__ __launch_bounds__(256) void ce16_col_combine_kernel(CeBufs b, Ce16Bufs c, int64_t n4, int ysplits, float d_loss, float* __restrict__ d_score) {
    const float sc = d_loss / b.nvalid[0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f4 v = ((const f4*)c.part_col)[i];
        for (int y = 1; y < ysplits; ++y) v += ((const f4*)c.part_col)[(int64_t)y * n4 + i];
        ((f4*)d_score)[i] = v * sc;
    }
}

// The route of one loss call: which kernels run its row pass (forward) and its row and column passes (backward).  Chosen once, by the
// forward call, from the dev switch ce_fast, the shape limits of the row-fixed kernels and C16_MIN_LOGITS; the backward call takes it
// from the forward's token.  ce_fast:
//   1 (default): one fused FWD + DPREC row pass (online softmax) and the cooperative column pass — on the 16-bit matrix cores with split
//      operands (ce16_*) from C16_MIN_LOGITS logits on, on the f32 cores below; 2: separate FWD and DPREC row passes (round-2a form); 0: the
//      plain kernel everywhere (per-logit work: slow); 3: ce16_* at every size; 4: the f32 fused passes at every size (test knobs)
enum { CE_ROUTE_GENERIC = 0,      // ce_pass_kernel for all three passes (any S <= 63)
       CE_ROUTE_ROWPASS = 1,      // ce_rowpass_kernel<CE_FWD>, <CE_DPREC>, ce_colpass_kernel
       CE_ROUTE_FUSED = 2,        // ce_rowpass_kernel<CE_FUSED> leaves d_prec for d_loss = 1 in the workspace; backward scales it + ce_colpass_kernel
       CE_ROUTE_SPLIT16 = 3 };    // ce16_*: as FUSED, on split fp16 operand images kept in the workspace
int g_ce_fast = 1;
// bs = 128 (1,280 x 1,408 logits): 29 us per f32 pass, launch-sized — the split route's four extra small launches would cost more than it gains
constexpr int64_t C16_MIN_LOGITS = (int64_t)1 << 24;
// EW: the embedding width.  The split-operand route is 64 wide: at EW > 64 its two cases take the f32 fused passes.
int ce_route(int64_t bs, int S, int EW) {
    // the row-fixed kernels keep a sequence's ids in registers / LDS, span at most four sequences per 16-row tile and index with 32 bits
    if (!g_ce_fast || S < 5 || S + 1 > MAXS1 || bs * (int64_t)(S + 1) >= (1ll << 31)) return CE_ROUTE_GENERIC;
    if (g_ce_fast == 3 || (g_ce_fast == 1 && bs * S * bs * (int64_t)(S + 1) >= C16_MIN_LOGITS)) return EW == E ? CE_ROUTE_SPLIT16 : CE_ROUTE_FUSED;
    return (g_ce_fast == 1 || g_ce_fast == 4) ? CE_ROUTE_FUSED : CE_ROUTE_ROWPASS;
}
// The run-time width as the EW template argument: f(integral_constant<int, 64 | 128 | 192 | 256>) — the widths `check` lets through
template <class F>
void with_ew(int EW, F&& f) {
    switch (EW) {
        case 64: f(std::integral_constant<int, 64>{}); break;
        case 128: f(std::integral_constant<int, 128>{}); break;
        case 192: f(std::integral_constant<int, 192>{}); break;
        default: f(std::integral_constant<int, 256>{});
    }
}
#define CE_EW decltype(ew)::value
// The run-time S + 1 as the RS1 template argument (slots per sequence compared per logit): f(integral_constant<int, 11 or MAXS1>).  11 is the
// reference's max_seq_len 10 + 1; every kernel's RS1 = 11 instantiation also handles shorter sequences.  The plain kernel has no such argument.
template <class F>
void with_rs1(int S, F&& f) {
    if (S + 1 <= 11) f(std::integral_constant<int, 11>{});
    else f(std::integral_constant<int, MAXS1>{});
}
#define CE_RS1 decltype(rs1)::value
// ranges of Y per X block: about seven workgroups per CU (four are resident at a time) and >= 8 steps per range.  Same-box sweep at bs = 1024
// (tools/ce_sweep.py, forward + backward of the loss, both passes with the same count): 4 ranges 402 - 407 us, 6 390, 8 365, 10 355 - 357,
// 11 347 - 348, 12 357, 16 353; the f32 passes 852 - 891.
int g_ce16_ys = 0;               // > 0: this many Y ranges (sweeps)
int ce16_ysplits(int64_t nx, int64_t ny, int nsub) {
    if (g_ce16_ys > 0) return g_ce16_ys > C16_MAX_YS ? C16_MAX_YS : g_ce16_ys;
    const int64_t xb = ceil_div(nx, (int64_t)64 * nsub), steps = ceil_div(ny, (int64_t)32), cus = iisan_cu_count();
    int64_t ys = (7 * cus + xb / 2) / xb;
    if (ys > C16_MAX_YS) ys = C16_MAX_YS;
    while (ys > 1 && steps / ys < 8) --ys;
    return ys < 1 ? 1 : (int)ys;
}
// one pass of the split-operand route over nx rows of X against ny rows of Y (COL: X = score rows, the backward's column pass); returns its Y ranges
template <bool COL, int NSUB>
int launch_ce16_pass_n(const float* log_mask, const CeBufs& b, const Ce16Bufs& c, int64_t bs, int S, hipStream_t s, int* ys_out) {
    const int64_t nx = COL ? bs * (S + 1) : bs * S, ny = COL ? bs * S : bs * (S + 1);
    const int ys = ce16_ysplits(nx, ny, NSUB);
    const int steps_per = (int)ceil_div(ceil_div(ny, (int64_t)32), (int64_t)ys);
    const dim3 grid((unsigned)ceil_div(nx, (int64_t)64 * NSUB), (unsigned)ys);
    with_rs1(S, [&](auto rs1) {
        if constexpr (COL) hipLaunchKernelGGL((ce16_colpass_kernel<CE_RS1, NSUB>), grid, dim3(256), 0, s, log_mask, b, c, (int)bs, S, steps_per);
        else hipLaunchKernelGGL((ce16_rowpass_kernel<CE_RS1, NSUB>), grid, dim3(256), 0, s, log_mask, b, c, (int)bs, S, steps_per);
    });
    IISAN_LAUNCH_OK();
    *ys_out = ys;
    return IISAN_OK;
}
int g_ce16_nsub = 1;             // X blocks of 16 rows per wave (1 or 2)
template <bool COL>
int launch_ce16_pass(const float* log_mask, const CeBufs& b, const Ce16Bufs& c, int64_t bs, int S, hipStream_t s, int* ys_out) {
    return g_ce16_nsub == 2 ? launch_ce16_pass_n<COL, 2>(log_mask, b, c, bs, S, s, ys_out) : launch_ce16_pass_n<COL, 1>(log_mask, b, c, bs, S, s, ys_out);
}

int check(int64_t bs, int S, int Ein) {
    IISAN_CHECK_SHAPE(bs > 0 && S >= 1 && S <= 63, "inbatch_ce: bs %lld / S %d unsupported", (long long)bs, S);
    IISAN_CHECK_SHAPE(Ein > 0 && Ein <= EMAX && Ein % 64 == 0, "inbatch_ce: embedding_dim must be 64, 128, 192 or 256 (got %d)", Ein);
    return IISAN_OK;
}

// the workspace of one call: the f32 passes' buffers, and at the width of the split-operand route (alone) that route's images and partials
void carve_all(WsCarver& c, CeBufs& b, Ce16Bufs& b16, int64_t bs, int S, int EW) {
    carve(c, b, bs, S, EW);
    if (EW == E) carve16(c, b16, bs, S);
}

}  // namespace

extern "C" size_t iisan_inbatch_ce_ws_bytes_e(int64_t bs, int32_t S, int32_t Ein) {
    if (bs <= 0 || S < 1 || S > 63 || Ein <= 0 || Ein > EMAX || Ein % 64) return 0;
    WsCarver c(nullptr, 0);
    CeBufs b;
    Ce16Bufs b16;
    carve_all(c, b, b16, bs, S, Ein);
    return c.off;
}
extern "C" size_t iisan_inbatch_ce_ws_bytes(int64_t bs, int32_t S) {
    WsCarver c(nullptr, 0);
    CeBufs b;
    Ce16Bufs b16;
    carve_all(c, b, b16, bs, S, E);
    return c.off;
}

// the forward call's token: a tag, the call shape (the width as EW / 64 - 1 in bits 48..55: 0 at 64) and the route it took (CE_ROUTE_*) —
// so that the backward call follows what THAT call did, not the dev switch's later value, and the library keeps no per-call state
static uint64_t ce_token(int64_t bs, int32_t S, int EW, int route) {
    return 0xCE00000000000000ull | ((uint64_t)(EW / 64 - 1) << 48) | ((uint64_t)(bs & 0xFFFFFFFFll) << 16) | ((uint64_t)(S & 0xFF) << 8) | (uint64_t)(route + 1);
}
IISAN_DEV_KNOB(ce_fast, g_ce_fast);
IISAN_DEV_KNOB(ce16_nsub, g_ce16_nsub);
IISAN_DEV_KNOB(ce16_ys, g_ce16_ys);
static int64_t g_cnt_ce16 = 0;            // forward calls on the split-operand route (route counter, common.h)
IISAN_DEV_COUNTER(ce16, g_cnt_ce16);

extern "C" int32_t iisan_inbatch_ce_route(int64_t bs, int32_t S) { return check(bs, S, E) == IISAN_OK ? ce_route(bs, S, E) : -1; }
extern "C" int32_t iisan_inbatch_ce_route_e(int64_t bs, int32_t S, int32_t Ein) {
    if (bs <= 0 || S < 1 || S > 63 || Ein <= 0 || Ein > EMAX || Ein % 64) return -1;      // (check() would leave an error message behind)
    return ce_route(bs, S, Ein);
}

extern "C" int iisan_inbatch_ce_fwd(const int64_t* ids, const float* score, const float* prec, const float* log_mask,
                                    const float* pop_prob, int64_t n_pop, int64_t bs, int32_t S, int32_t Ein, float* loss,
                                    void* ws, size_t ws_bytes, uint64_t* fwd_token, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    IISAN_TRY(check(bs, S, Ein));
    IISAN_CHECK_SHAPE(n_pop > 0, "inbatch_ce_fwd: empty pop_prob table");
    WsCarver c(ws, ws_bytes);
    CeBufs b;
    Ce16Bufs b16;
    carve_all(c, b, b16, bs, S, Ein);
    if (c.overflow || !ws) {
        iisan_set_error("inbatch_ce_fwd: workspace too small (%zu < %zu)", ws_bytes, c.off);
        return IISAN_EWORKSPACE;
    }
    const int64_t T = bs * S, M = bs * (S + 1);
    const dim3 rows((unsigned)ceil_div(T, 16));
    hipLaunchKernelGGL(ce_prep_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, s, ids, log_mask, pop_prob, n_pop, b, bs, S);
    IISAN_LAUNCH_OK();
    hipLaunchKernelGGL(ce_count_kernel, dim3(1), dim3(256), 0, s, log_mask, T, b.nvalid);
    IISAN_LAUNCH_OK();
    IISAN_CHECK_SHAPE(fwd_token != nullptr, "inbatch_ce_fwd: fwd_token must not be null");
    const int route = ce_route(bs, S, Ein);
    *fwd_token = ce_token(bs, S, Ein, route);
    float* const none = nullptr;
    switch (route) {
        case CE_ROUTE_SPLIT16: {     // amax -> images -> fused row pass per Y range -> combine (lse, row loss, d_prec for d_loss = 1 in the workspace)
            ++g_cnt_ce16;
            IISAN_HIP_OK(hipMemsetAsync(b16.amax, 0, 16, s));
            hipLaunchKernelGGL(ce16_amax_kernel, dim3(64, 2), dim3(256), 0, s, prec, T * E, score, M * E, b16.amax);
            IISAN_LAUNCH_OK();
            hipLaunchKernelGGL(ce16_split_kernel, dim3((unsigned)ceil_div(M, 32), 2), dim3(256), 0, s, prec, T, score, M, b16);
            IISAN_LAUNCH_OK();
            int ys = 1;
            IISAN_TRY(launch_ce16_pass<false>(log_mask, b, b16, bs, S, s, &ys));
            hipLaunchKernelGGL(ce16_row_combine_kernel, dim3((unsigned)ceil_div(T * E, 256)), dim3(256), 0, s, log_mask, b, b16, (int)bs, S, ys);
            break;
        }
        case CE_ROUTE_FUSED:         // the forward pass leaves d_prec (for d_loss = 1) in the workspace, the backward call only scales it
            with_ew(Ein, [&](auto ew) { with_rs1(S, [&](auto rs1) { hipLaunchKernelGGL((ce_rowpass_kernel<CE_FUSED, CE_RS1, CE_EW>), rows, dim3(256), 0, s, prec, score, log_mask, b, (int)bs, S, 0.f, none); }); });
            break;
        case CE_ROUTE_ROWPASS:
            with_ew(Ein, [&](auto ew) { with_rs1(S, [&](auto rs1) { hipLaunchKernelGGL((ce_rowpass_kernel<CE_FWD, CE_RS1, CE_EW>), rows, dim3(256), 0, s, prec, score, log_mask, b, (int)bs, S, 0.f, none); }); });
            break;
        default:
            with_ew(Ein, [&](auto ew) { hipLaunchKernelGGL((ce_pass_kernel<CE_FWD, CE_EW>), rows, dim3(256), 0, s, prec, score, log_mask, b, bs, S, 0.f, none); });
    }
    IISAN_LAUNCH_OK();
    hipLaunchKernelGGL(ce_reduce_kernel, dim3(1), dim3(256), 0, s, b.rowloss, T, b.nvalid, loss);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

extern "C" int iisan_inbatch_ce_bwd(const int64_t* ids, const float* score, const float* prec, const float* log_mask,
                                    const float* pop_prob, int64_t bs, int32_t S, int32_t Ein, float d_loss, float* d_score,
                                    float* d_prec, void* ws, size_t ws_bytes, uint64_t fwd_token, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    IISAN_TRY(check(bs, S, Ein));
    WsCarver c(ws, ws_bytes);
    CeBufs b;
    Ce16Bufs b16;
    carve_all(c, b, b16, bs, S, Ein);      // ids32/debias/colpad/lse/nvalid were filled by the forward call on the same workspace, and, on
                                           // the split-operand route, the operand images and their amax
    if (c.overflow || !ws) {
        iisan_set_error("inbatch_ce_bwd: workspace too small (%zu < %zu)", ws_bytes, c.off);
        return IISAN_EWORKSPACE;
    }
    const int64_t T = bs * S, M = bs * (S + 1);
    const dim3 rows((unsigned)ceil_div(T, 16)), cols((unsigned)ceil_div(M, 16));
    int route = -1;           // the forward's, whatever the dev switch says by now: what this route needs is in the workspace
    for (int r = CE_ROUTE_GENERIC; r <= CE_ROUTE_SPLIT16; ++r)
        if (fwd_token == ce_token(bs, S, Ein, r)) route = r;
    if (route == CE_ROUTE_SPLIT16 && Ein != E) route = -1;      // (no forward call returns it)
    if (route < 0) {
        iisan_set_error("inbatch_ce_bwd: fwd_token %llx is not what inbatch_ce_fwd returns for bs = %lld, S = %d, embedding_dim = %d", (unsigned long long)fwd_token, (long long)bs, S, Ein);
        return IISAN_EBADSHAPE;
    }
    // d_prec: scaled from the forward's d_prec for d_loss = 1, or its own row pass
    if (route == CE_ROUTE_FUSED || route == CE_ROUTE_SPLIT16)
        hipLaunchKernelGGL(ce_scale_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(T * Ein / 4, 256), 1024)), dim3(256), 0, s, b.dprec, d_loss, d_prec, T * Ein / 4);
    else if (route == CE_ROUTE_ROWPASS)
        with_ew(Ein, [&](auto ew) { with_rs1(S, [&](auto rs1) { hipLaunchKernelGGL((ce_rowpass_kernel<CE_DPREC, CE_RS1, CE_EW>), rows, dim3(256), 0, s, prec, score, log_mask, b, (int)bs, S, d_loss, d_prec); }); });
    else
        with_ew(Ein, [&](auto ew) { hipLaunchKernelGGL((ce_pass_kernel<CE_DPREC, CE_EW>), rows, dim3(256), 0, s, prec, score, log_mask, b, bs, S, d_loss, d_prec); });
    IISAN_LAUNCH_OK();
    // d_score: the column pass
    if (route == CE_ROUTE_SPLIT16) {
        int ys = 1;
        IISAN_TRY(launch_ce16_pass<true>(log_mask, b, b16, bs, S, s, &ys));
        hipLaunchKernelGGL(ce16_col_combine_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(M * E / 4, 256), 2048)), dim3(256), 0, s, b, b16, M * E / 4, ys, d_loss, d_score);
    } else if (route != CE_ROUTE_GENERIC) {
        with_ew(Ein, [&](auto ew) { with_rs1(S, [&](auto rs1) { hipLaunchKernelGGL((ce_colpass_kernel<CE_RS1, CE_EW>), cols, dim3(256), 0, s, prec, score, log_mask, b, (int)bs, S, d_loss, d_score); }); });
    } else {
        with_ew(Ein, [&](auto ew) { hipLaunchKernelGGL((ce_pass_kernel<CE_DSCORE, CE_EW>), cols, dim3(256), 0, s, prec, score, log_mask, b, bs, S, d_loss, d_score); });
    }
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}
