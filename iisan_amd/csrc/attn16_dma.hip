// ViT self-attention (no key_bias, 192 < S <= 208: 13 key tiles of 16) with K and V staged by LDS-DMA and V read transposed.
// Same input / output layout and the same per-block arithmetic as attention16_kernel<T, 13, true, false> (attn16.hip): S^T = K · Q^T on
// 16x16x32, last-tile limit through fmed3, exp2 with the folded 1/8 scale, fp32 row sums of the unrounded P, P rounded to the operand
// type, 16-key tail product.  What differs is how the operands travel:
//   * K and V of a head go from global memory into LDS by `global_load_lds_dwordx4` (dma16 below: 1 KiB = 8 rows per wave-instruction, no VGPR
//     round trip, no staging instructions).  The destination of a piece is lane-linear, so both swizzles live in each lane's SOURCE
//     address: K chunk c (16 bytes) of row r sits at slot c ^ (r & 7) as before; V chunk c of row r sits at slot c ^ (2 ((r >> 1) & 3)).
//     Rows at or beyond S fetch row S - 1 (finite data under P = 0; a read past the head's block would leave the tensor for the last item).
//   * V stays ROW-MAJOR in LDS.  The A operand of O^T = V^T · P^T is read with `ds_read_b64_tr_b16`: lane group g of 16 lanes takes the
//     4 keys x 16 head dims block of keys 32 kb + 4 g + (0..3) (then + 16): lane 4 q + p of the group addresses row q, dims 4 p .. 4 p + 3,
//     lane i receives dim i of the four keys — elements 0..3 (4..7) of the fragment, the k-slots P already occupies in registers.
//     Banks (64 x 4 bytes for this read, counted per 32-lane half): a half reads 8 consecutive rows x 32 bytes; rows of equal parity share
//     their 128-byte half of the bank space, and the V swizzle sends the four of them to four different 32-byte column pairs: all 64 banks once.
//   * one workgroup = one (item, head), K and V single-buffered: 53,248 B of LDS and 168 registers, so THREE workgroups share a CU and
//     the loads of one run under the arithmetic of the other two — the three-workgroup form of round 4 without its staging instructions.
//     (Measured against it and removed: two to six heads per workgroup over three rotating buffers, two workgroups per CU, the next head's K
//     landing during this head's blocks — profiles/attention_dma.md.)  V is first needed after the first block's softmax (one barrier there).
//   * Q: two 16-byte loads per lane per block into 8 fixed registers, requested one block ahead (inline asm, waited for by hand: hipcc's own
//     wait for a plain load does not know the LDS-DMA pieces issued behind it and drains them — gemm16_h256.hip, stream_load).
// vmcnt retires in order and DMA pieces, Q loads and context stores share it; every wait below is `vmcnt(n)` with n = the number of
// vector-memory instructions the wave has issued BEHIND the one it needs (a lower bound where waves differ), so that the two context
// stores of the previous block stay in flight over it.  The counts are written next to each wait.
#include "attn16_block.h"

static int g_attn_route = 0;            // 0 = this kernel where it applies by default, 1 = always attention16_kernel, 2 = this kernel wherever it applies
IISAN_DEV_KNOB(attn_route, g_attn_route);
static int64_t g_attn16_dma_count = 0;
IISAN_DEV_COUNTER(attn16_dma, g_attn16_dma_count);

namespace {

constexpr int DMA_NT16 = 13, DMA_SP = DMA_NT16 * 16;       // 208 key slots
constexpr int DMA_BUF = DMA_SP * 128;                        // one head's K or V: 26,624 B = 26 pieces of 1 KiB
constexpr int DMA_PIECES = DMA_BUF / 1024;
constexpr int DMA_LDS = 2 * DMA_BUF;                         // K, then V

#define DMA_FENCE() __builtin_amdgcn_sched_barrier(0)
// vmcnt(n) as the builtin (gfx9 encoding: vmcnt[3:0] | expcnt << 4 | lgkmcnt << 8 | vmcnt[5:4] << 14)
#define DMA_VMCNT(n)                                                                               \
    do {                                                                                           \
        DMA_FENCE();                                                                               \
        __builtin_amdgcn_s_waitcnt(((n) & 15) | (7 << 4) | (15 << 8) | ((((n) >> 4) & 3) << 14));  \
        DMA_FENCE();                                                                               \
    } while (0)
// every LDS read of the wave has been consumed by an MFMA before it arrives here; the DMA pieces are waited for by count in front
#define DMA_BARRIER()                                    \
    do {                                                 \
        DMA_FENCE();                                     \
        asm volatile("s_barrier" ::: "memory");          \
        DMA_FENCE();                                     \
    } while (0)

// One LDS-DMA piece: 16 bytes per lane from base + lane_off into LDS at lds_dst + 16 lane (M0 = the wave-uniform LDS address).  Inline asm, not
// glds16: with the builtin hipcc knows the piece as a pending LDS write and puts `s_waitcnt vmcnt(0)` in front of the first transposed read behind
// it (the intrinsic of `ds_read_b64_tr_b16` is not a plain LDS load to its wait insertion) — a wait for the NEXT head's K in the middle of a
// block.  M0 is written and restored inside the one statement (the compiler reserves it).
__device__ __forceinline__ void dma16(unsigned lane_off, const void* base, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_off), "s"(lds_dst), "s"(base) : "memory");
}

template <typename T>
__global__ __launch_bounds__(256, 3) void attention16_dma_kernel(const typename T::elem* __restrict__ qkv, typename T::elem* __restrict__ ctx,
                                                                 int S, int heads) {
    typedef typename T::v8 V8;
    typedef typename T::v4 V4;
    typedef short s4 __attribute__((ext_vector_type(4)));
    constexpr int NT16 = DMA_NT16;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform for the compiler too: EXEC stays all ones around the transposed reads
    const int item = blockIdx.x / heads, h = blockIdx.x - item * heads;
    const int D = heads * 64;
    const int j = lane & 15, g = lane >> 4;

    // ---- LDS-DMA: piece pc = rows 8 pc .. 8 pc + 7 of a head's K or V; lane l writes row 8 pc + (l >> 3), slot l & 7 ----
    const int prow = lane >> 3;
    const unsigned ksrc = (unsigned)(((lane & 7) ^ prow) << 4);                       // K: slot = chunk ^ (row & 7)
    const unsigned vsrc = (unsigned)(((lane & 7) ^ (((lane >> 4) & 3) << 1)) << 4);   // V: slot = chunk ^ (2 ((row >> 1) & 3))
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const char* hb = (const char*)(qkv + (int64_t)blockIdx.x * 3 * S * 64);          // this head's [q | k | v][S][64]
    // pieces w0, w0 + 4, ... < 26 of one operand: 7 for w0 < 2, 6 otherwise
    auto dma_operand = [&](const char* src, unsigned lane_src, int dst, int w0) {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
            const int pc = w0 + 4 * i;
            if (pc < DMA_PIECES) {
                int r = pc * 8 + prow;
                r = r < S ? r : S - 1;
                dma16((unsigned)(r * 128) + lane_src, src, lds0 + dst + pc * 1024);
            }
        }
    };
    // Q of one 16-query block: rows clamped to S - 1, lane (j, g) takes dims 8 g .. 8 g + 7 and 32 + 8 g .. 32 + 8 g + 7
    // The loads land in FIXED registers, v[160:167], named in the asm text and in its clobber list, requested a whole block ahead; at the top of a
    // block, behind the counted wait, take_q copies them into registers of the compiler's choice.  As asm OUTPUT operands the destinations were
    // ordinary values to hipcc: the statements of different blocks got different registers, joined by `v_mov` copies where the blocks of a multi-head form of this kernel met —
    // copies of registers whose load was still in flight (run-to-run differences in the outputs).  Nothing tells the register allocator to stay away
    // from v[160:167] between a request and its take_q; the kernel needs about 150 registers, and tests/test_isa_screen_attention_dma.py fails when a
    // compiler-generated instruction touches v160 or above.  168 registers still fit three waves per SIMD.
    // (take_q is inline-asm VALU: it reads registers a load wrote, behind the wait, and stands where every MFMA of the previous block has retired —
    // their results went through the conversions of the context store — so it needs nothing from the hazard recognizer.)
#define DMA_QREGS "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167"
    auto load_q = [&](int qb) {
        int sq = qb * 16 + j;
        sq = sq < S ? sq : S - 1;
        const unsigned off = (unsigned)(sq * 128 + g * 16);
        DMA_FENCE();
        asm volatile("global_load_dwordx4 v[160:163], %0, %1\n\tglobal_load_dwordx4 v[164:167], %0, %1 offset:64"
                     : : "v"(off), "s"(hb) : "memory", DMA_QREGS);
        DMA_FENCE();
    };
    auto take_q = [&](V8 (&qf)[2]) {
        u2 a, b, c, d;
        DMA_FENCE();
        asm volatile("v_mov_b64 %0, v[160:161]\n\tv_mov_b64 %1, v[162:163]\n\tv_mov_b64 %2, v[164:165]\n\tv_mov_b64 %3, v[166:167]"
                     : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d) : : "memory");
        DMA_FENCE();
        qf[0] = __builtin_bit_cast(V8, (u4){a[0], a[1], b[0], b[1]});
        qf[1] = __builtin_bit_cast(V8, (u4){c[0], c[1], d[0], d[1]});
    };

    // the last tile's per-key limit: +inf keeps, -inf removes a pad slot (keys 192 + 4 g + r)
    f4 lim;
#pragma unroll
    for (int r = 0; r < 4; ++r) lim[r] = (NT16 - 1) * 16 + g * 4 + r >= S ? -INFINITY : INFINITY;

    // transposed V reads: lane 4 q + p of group g addresses key row 4 g + q (+ 32 kb, + 16), dims 16 dt + 4 p .. + 3
    unsigned vaddr[4];
    {
        const int q = (lane >> 2) & 3, p = lane & 3, rowl = 4 * g + q;
        const int swz = ((rowl >> 1) & 3) << 1;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) vaddr[dt] = (unsigned)(rowl * 128 + (((2 * dt + (p >> 1)) ^ swz) << 4) + 8 * (p & 1));
    }
    const unsigned kaddr0 = (unsigned)(j * 128 + ((g ^ (j & 7)) << 4)), kaddr1 = (unsigned)(j * 128 + (((4 + g) ^ (j & 7)) << 4));

    // in this order: K (7 / 6 pieces per wave), Q of the wave's first block (2 loads), V (7 / 6)
    dma_operand(hb + (int64_t)S * 128, ksrc, 0, wave);
    load_q(wave);
    dma_operand(hb + (int64_t)2 * S * 128, vsrc, DMA_BUF, wave);
    const char* sK = smem;
    const char* sV = smem + DMA_BUF;

    DMA_VMCNT(6);                               // K and Q: behind them, at least 6 V pieces
    DMA_BARRIER();                              // every wave's K pieces are in LDS
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int qb = wave + 4 * i;
        if (qb >= NT16) break;
        if (i >= 1) DMA_VMCNT(2);          // this block's Q: requested at the top of the previous block, that block's two stores behind it
        V8 qf[2];
        take_q(qf);
        if (qb + 4 < NT16) load_q(qb + 4);     // the next block's Q
        const int sq = qb * 16 + j;

        // S^T tiles: lane holds query j, keys 16 t + 4 g + r (raw dot products; the 1/8 scale is folded into exp2)
        f4 sc[NT16];
        {
            constexpr int KBATCH = 4;
#pragma unroll
            for (int t0 = 0; t0 < NT16; t0 += KBATCH) {
                V8 kf[KBATCH][2];
#pragma unroll
                for (int u = 0; u < KBATCH; ++u)
                    if (t0 + u < NT16) {
                        kf[u][0] = *(const V8*)(sK + (t0 + u) * 2048 + kaddr0);
                        kf[u][1] = *(const V8*)(sK + (t0 + u) * 2048 + kaddr1);
                    }
                DMA_FENCE();
#pragma unroll
                for (int u = 0; u < KBATCH; ++u) {
                    if (t0 + u >= NT16) continue;
                    f4 acc = {0.f, 0.f, 0.f, 0.f};
                    acc = T::mfma(kf[u][0], qf[0], acc);
                    acc = T::mfma(kf[u][1], qf[1], acc);
                    sc[t0 + u] = acc;
                }
            }
        }
        attn_apply_key_limit(sc[NT16 - 1], lim);
        const float inv = attn_row_softmax(sc, AttnKeepAll());

        if (i == 0) {
            // V: own pieces landed, then everybody's.  Behind the wave's V pieces: the two Q loads of block 1.
            DMA_VMCNT(2);
            DMA_BARRIER();
        }

        // O^T = V^T · P^T, the V fragments read transposed out of the row-major image
        f4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = (f4){0.f, 0.f, 0.f, 0.f};
        {
            auto vtr = [&](int dt, int byte_off) {
                return __builtin_bit_cast(V4, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                                  (__attribute__((address_space(3))) s4*)(sV + vaddr[dt] + byte_off)));
            };
            auto vload = [&](int kb, V8 (&vf)[4]) {
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
                    vf[dt] = __builtin_shufflevector(vtr(dt, kb * 4096), vtr(dt, kb * 4096 + 2048), 0, 1, 2, 3, 4, 5, 6, 7);
            };
            V8 vc[4];
            vload(0, vc);
            constexpr int NPV = NT16 / 2;
#pragma unroll
            for (int kb = 0; kb < NPV; ++kb) {
                V8 vn[4];
                if (kb + 1 < NPV) vload(kb + 1, vn);
                const V8 pf = attn_round_p<T>(sc[2 * kb], sc[2 * kb + 1]);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = T::mfma(vc[dt], pf, o[dt]);
                if (kb + 1 < NPV) {
#pragma unroll
                    for (int dt = 0; dt < 4; ++dt) vc[dt] = vn[dt];
                }
            }
            const V4 pt = attn_round_p_tail<T>(sc[NT16 - 1]);      // keys 192 .. 207
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) o[dt] = Mfma16k16<T>::run(vtr(dt, (NT16 / 2) * 4096), pt, o[dt]);
        }
        // exactly two store instructions per block (every block of 192 < S <= 208 has a real query): the waits above count them
        attn_store_ctx<T>(ctx + (size_t)item * S * D, sq * D + h * 64, [&] { return g; }, o, inv, sq < S);
        DMA_FENCE();
    }
}

template <typename T>
int launch_dma_t(const void* qkv, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    typedef typename T::elem E;
    static OncePerDevice raised;
    if (raised.first())
        IISAN_HIP_OK(hipFuncSetAttribute((const void*)attention16_dma_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, DMA_LDS));
    dim3 grid((unsigned)(items * heads)), block(256);
    hipLaunchKernelGGL((attention16_dma_kernel<T>), grid, block, DMA_LDS, s, (const E*)qkv, (E*)ctx, S, heads);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

}  // namespace

bool attention16_dma_applicable(const float* key_bias, int S) { return key_bias == nullptr && S > 192 && S <= 208; }

// the route of launch_attention16 (attn16.hip) for this problem under the dev switch attn_route
bool attention16_dma_routed(const float* key_bias, int S) {
    return g_attn_route != 1 && attention16_dma_applicable(key_bias, S);
}

int launch_attention16_dma(int dtype16, const void* qkv, void* ctx, int64_t items, int S, int heads, hipStream_t s) {
    IISAN_CHECK_SHAPE(attention16_dma_applicable(nullptr, S), "attention16_dma: sequence length %d outside 193..208", S);
    // the last DMA piece of the last item must end inside the tensor: rows are clamped to S - 1, chunks stay inside their row
    IISAN_CHECK_SHAPE((int64_t)S * 128 * 3 < (1ll << 31), "attention16_dma: head block too large");
    ++g_attn16_dma_count;
    return dtype16 == IISAN_BF16 ? launch_dma_t<BF16>(qkv, ctx, items, S, heads, s) : launch_dma_t<F16>(qkv, ctx, items, S, heads, s);
}
