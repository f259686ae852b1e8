// Third-generation 16-bit MFMA GEMM: persistent 256x256x64 tiles with two STAGGERED wave groups.
//
// Ablation of the second generation (lock-step 256x256 tiles): with DMA and epilogue removed its K loop still reached only
// 55 % of the MFMA peak — all 8 waves read their fragments from LDS at the same time and then all issue MFMAs at the
// same time, so the two waves sharing a SIMD never overlap (LDS-read phase: matrix pipe idle; MFMA phase: LDS idle).
//
// Here the workgroup is split into two groups of four waves, A (rows 0..127 of the tile; waves 4..7) and B (rows
// 128..255; waves 0..3); waves w and w+4 share a SIMD.  Time is cut into SLOTS separated by one `s_barrier`; each group
// alternates a READ slot R(s) (24 ds_read_b128: every fragment of K-step s into registers) and an MFMA slot M(s)
// (32 x v_mfma_f32_32x32x16), and B runs ONE SLOT BEHIND A:
//
//        slot:   2s        2s+1       2s+2       2s+3
//        A:      R(s)      M(s)       R(s+1)     M(s+1)
//        B:      M(s-1)    R(s)       M(s)       R(s+1)
//
// so on every SIMD one wave feeds the matrix pipe while its sibling reads LDS.
//
// Where the LDS-DMA goes was settled with tools/micro/slot_dma.hip (cycles per K-step on one CU, 2048 = MFMA bound):
//   8 `global_load_lds` per wave at the head of the read slot 3592, after the ds_reads 2754, 4 + 4 split 2741,
//   ALL 8 INTERLEAVED WITH THE MFMAs (one after every 4) AND WAITED FOR ONE SLOT LATER: 2168.
// What costs is a wave waiting for its own loads or queueing at the texture addresser next to ds_reads, not the issue
// among MFMAs.  So read slots hold only the 24 ds_reads plus the wait, MFMA slots issue the DMA, and every piece has a
// full slot between its issue and its wait:
//        A in M(s)   (slot 2s+1) : B's A-operand half of step s+1 (read in slot 2s+3), A's own half of step s+2 (2s+4)
//        B in M(s)   (slot 2s+2) : the whole W tile of step s+2   (read in slots 2s+4, 2s+5)
//        A and B: `s_waitcnt vmcnt(0)` at the END of each read slot (so the stores of an epilogue get a slot as well)
// Each ring buffer was last read at least one slot before it is overwritten (2 stages of 64 KiB).
//
// This kernel is also the race screen of gemm16_h256.hip (dev switch gemm16_variant = 3) and serves the shapes
// gemm16_h256_applicable() turns down.  What the two share lives ONCE, in gemm16_t256.h: tile constants, the MFMA with swapped
// operands, the W-row permutation, the fences (and why the compiler needs them), the fragment reads, the DMA plan of an MFMA slot
// with its inline-asm piece, the full MFMA step, the host's grid rule.
// This file's own: the slot program above (groups A and B), the row-major tile walk (make_plan divides the flat step by nk), the
// plain 16-bit epilogue with slots of its own, the timeline hooks, the inline-asm wait macros — and its copy of the lane staging
// offsets with vj, the prologue pieces and the accumulator / fragment-offset set-up, which gemm16_h256.hip repeats (gemm16_t256.h
// says why).
#include "gemm16_t256.h"

namespace {

#define S256_VMCNT(n)                                        \
    do {                                                     \
        S256_FENCE();                                        \
        asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory"); \
        S256_FENCE();                                        \
    } while (0)
#define S256_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

template <typename T, int EPI>
__global__ __launch_bounds__(512, 2) void gemm16_s256_kernel(Gemm16Args p, int tiles_m, int tiles_n) {
    typedef typename T::v8 V8;
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 * S_STAGE_BYTES ring + N floats of bias
    float* sBias = (float*)(smem + 2 * S_STAGE_BYTES);
    const uint32_t smem_lds = (uint32_t)(uintptr_t)smem;      // LDS byte address of the dynamic segment

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // 0 = A (tile rows 0..127), 1 = B (rows 128..255).  The YOUNGER half of the workgroup (waves 4..7) is group A: on every
    // SIMD the younger wave loses arbitration to its older sibling, so its MFMA slot runs longer (slot timelines: 1,640 vs
    // 1,252 cycles with the older waves as A; 1,400 vs 1,276 this way round) — it gets the lighter DMA duty (A-operand
    // halves; group B streams the W tile that every CU hammers) and the leading position.
    const int grp = 1 - (wave >> 2);
    const int wq = wave & 3;              // wave within the group = its 64-column slice of the tile

    const int G = gridDim.x;
    const int pid = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);
    const int ntiles = tiles_m * tiles_n;
    const int my_tiles = pid < ntiles ? (ntiles - pid + G - 1) / G : 0;
    const int nk = p.K / SBK;
    const int nsteps = my_tiles * nk;
    if (nsteps == 0) return;

    // staging offsets, kept to 5 VGPRs: lane -> row-in-chunk r8 = lane>>3, physical slot lane&7; the logical slot is
    // physical ^ ((row>>1)&7) = s0 ^ 4*(j&1) for chunk j of a 32-row-aligned run, s0 = (lane&7) ^ (lane>>4).
    const int r8 = lane >> 3;
    const int s0 = (lane & 7) ^ (lane >> 4);
    const int slotx0 = s0 * 16, slotx1 = (s0 ^ 4) * 16;
    const int rowA = r8 * p.lda * 2;                                             // A-operand: LDS row == global row
    const int rowW = (16 * ((r8 >> 2) & 1) + (r8 & 3)) * p.ldw * 2;              // W: permuted rows (nperm32s)
    const char* Abase = (const char*)p.A;
    const char* Wbase = (const char*)p.W;

    // One 1-KiB piece (8 LDS rows) of the A-operand half `h` / the W half `h` of flat step s; wave wq owns rows
    // h*128 + wq*32 .. +31 of a half, piece j = rows +8j.
    auto piece_A = [&](int s, int h, int j) {
        const int ti = s / nk, kt = s - ti * nk;
        const int tau = pid + ti * G;
        const int tm = tau / tiles_n;
        const int q0 = h * 128 + wq * 32;
        const char* Ag = Abase + (((int64_t)tm * SBM + q0 + 8 * j) * p.lda + (int64_t)kt * SBK) * 2 + rowA;
        glds16(Ag + ((j & 1) ? slotx1 : slotx0), smem + (s & 1) * S_STAGE_BYTES + (q0 + 8 * j) * 128);
    };
    auto piece_W = [&](int s, int h, int j) {   // LDS rows q0+8j.. hold W rows q0 + 4j + {0,16} + {0..3} (nperm32s)
        const int ti = s / nk, kt = s - ti * nk;
        const int tau = pid + ti * G;
        const int tm = tau / tiles_n, tn = tau - tm * tiles_n;
        const int q0 = h * 128 + wq * 32;
        const char* Wg = Wbase + (((int64_t)tn * SBN + q0 + 4 * j) * p.ldw + (int64_t)kt * SBK) * 2 + rowW;
        glds16(Wg + ((j & 1) ? slotx1 : slotx0), smem + (s & 1) * S_STAGE_BYTES + S_OP_BYTES + (q0 + 8 * j) * 128);
    };

    f16v acc[4][2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int frow = lane & 31, fh = lane >> 5;
    const int fsw = (frow >> 1) & 7;
    int xoff[4], woff2[2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) xoff[mi] = (grp * 128 + mi * 32 + frow) * 128;   // group g reads only its A-half
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) woff2[ni] = (wq * 64 + ni * 32 + frow) * 128;

    V8 wf[2][4], xf[4][4];
    auto read_step = [&](int s) { t256_read<V8, 0, 4, true, false>(smem, s, wf, xf, xoff, woff2, fh, fsw); };
    // per-lane source offset of piece j (j = pc & 3): row-in-chunk and swizzled 16-B slot, plus j chunks of 8 (A operand)
    // or 4 (permuted W) rows
    uint32_t vj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        vj[j] = (uint32_t)((grp == 0 ? rowA : rowW) + ((j & 1) ? slotx1 : slotx0)) + (uint32_t)j * (grp == 0 ? 8u * p.lda * 2u : 4u * p.ldw * 2u);
    // DMA plan (T256Plan) of the MFMA slot of flat step s; past the workgroup's last step it re-loads the last step
    auto make_plan = [&](int s) {
        T256Plan q;
        const int last = nsteps - 1;
        uint64_t g1, g2;
        if (grp == 0) {
            const int s1 = s + 1 < last ? s + 1 : last, s2 = s + 2 < last ? s + 2 : last;
            const int ti1 = s1 / nk, kt1 = s1 - ti1 * nk, tm1 = (pid + ti1 * G) / tiles_n;
            const int ti2 = s2 / nk, kt2 = s2 - ti2 * nk, tm2 = (pid + ti2 * G) / tiles_n;
            g1 = (uint64_t)Abase + (((int64_t)tm1 * SBM + 128 + wq * 32) * p.lda + (int64_t)kt1 * SBK) * 2;
            g2 = (uint64_t)Abase + (((int64_t)tm2 * SBM + wq * 32) * p.lda + (int64_t)kt2 * SBK) * 2;
            q.l1 = ((s + 1) & 1) * S_STAGE_BYTES + (128 + wq * 32) * 128;
            q.l2 = (s & 1) * S_STAGE_BYTES + (wq * 32) * 128;
        } else {
            const int s2 = s + 2 < last ? s + 2 : last;
            const int ti = s2 / nk, kt = s2 - ti * nk;
            const int tau = pid + ti * G;
            const int tm = tau / tiles_n, tn = tau - tm * tiles_n;
            g1 = (uint64_t)Wbase + (((int64_t)tn * SBN + wq * 32) * p.ldw + (int64_t)kt * SBK) * 2;
            g2 = g1 + (uint64_t)128 * p.ldw * 2;
            q.l1 = (s & 1) * S_STAGE_BYTES + S_OP_BYTES + (wq * 32) * 128;
            q.l2 = q.l1 + 128 * 128;
        }
        q.g1lo = t256_sgpr((uint32_t)g1); q.g1hi = t256_sgpr((uint32_t)(g1 >> 32));
        q.g2lo = t256_sgpr((uint32_t)g2); q.g2hi = t256_sgpr((uint32_t)(g2 >> 32));
        q.l1 = t256_sgpr(q.l1); q.l2 = t256_sgpr(q.l2);
        return q;
    };
    bool stores16 = false;     // the last epilogue issued exactly 16 store instructions per wave (full row tile, stores enabled)
    auto epilogue = [&](int s, int half) {
        const int ti = s / nk;
        const int tau = pid + ti * G;
        const int tm = tau / tiles_n, tn = tau - tm * tiles_n;
        stores16 = ((int64_t)(tm + 1) * SBM <= p.M) && !(p.debug & 1);
        // head-major QKV: this wave's 64 columns are one (q|k|v, head) pair -> wave-uniform; (item, token) of a row by
        // ONE 32-bit division per tile, then advanced by 32 rows per block (a 64-bit division per block cost ~800
        // VALU instructions per tile and wave)
        unsigned qk_which = 0, qk_hd = 0, qk_item = 0, qk_tok = 0;
        const unsigned qk_S = (unsigned)p.qkv_S;
        if constexpr (EPI == EPI_QKVH16) {
            const unsigned Dm = (unsigned)p.qkv_heads * 64u, n64 = (unsigned)(tn * SBN + wq * 64);
            const unsigned wq_ = n64 / Dm;
            qk_hd = (n64 - wq_ * Dm) >> 6;
            qk_which = wq_ + (unsigned)p.qkv_which0;
            const unsigned m0 = (unsigned)(tm * SBM + grp * 128 + half * 64 + frow);
            qk_item = m0 / qk_S;
            qk_tok = m0 - qk_item * qk_S;
        }
        // the lane's 32 bias values (its columns are the same for every 32-row block) are read from LDS ONCE per epilogue
        // half, up front — read inside the block loop, each block's four reads sat right before their adds behind an
        // lgkmcnt(0) (ISA): eight exposed LDS round trips per epilogue half
        f4 bbv[2][4];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4)
                bbv[ni][q4] = p.bias ? *(const f4*)(sBias + tn * SBN + wq * 64 + ni * 32 + 16 * fh + 4 * q4) : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            if ((mi >> 1) != half) continue;
            const int64_t m = (int64_t)tm * SBM + grp * 128 + mi * 32 + frow;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const int n = tn * SBN + wq * 64 + ni * 32 + 16 * fh;
                float v[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) v[r] = acc[mi][ni][r];
                if (m >= p.M || (p.debug & 1)) continue;

                typename T::elem* op;
                if constexpr (EPI == EPI_QKVH16) {
                    op = (typename T::elem*)p.out + ((((int64_t)qk_item * p.qkv_heads + qk_hd) * 3 + qk_which) * qk_S + qk_tok) * 64 + (ni * 32 + 16 * fh);
                } else {
                    op = (typename T::elem*)p.out + m * p.ldo + n;
                }
                f2 g[8];       // bias added pairwise: v_pk_add_f32 (8 instead of 16 v_add_f32 per block)
#pragma unroll
                for (int k = 0; k < 8; ++k) g[k] = (f2){v[2 * k], v[2 * k + 1]} + (f2){bbv[ni][k >> 1][2 * (k & 1)], bbv[ni][k >> 1][2 * (k & 1) + 1]};
                if constexpr (EPI == EPI_GELU16) gelu_erf_fast2x8(g);
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    V8 o;
#pragma unroll
                    for (int e = 0; e < 8; e += 2) {
                        o[e] = T::from_f32(g[4 * h2 + e / 2][0]);
                        o[e + 1] = T::from_f32(g[4 * h2 + e / 2][1]);
                    }
                    *(V8*)(op + 8 * h2) = o;
                }
            }
            if constexpr (EPI == EPI_QKVH16) {
                qk_tok += 32;
                while (qk_tok >= qk_S) { qk_tok -= qk_S; ++qk_item; }
            }
        }
        // the accumulators are dead now (the next K-step is a tile's first and starts from C = 0); an empty asm that
        // "defines" them tells the register allocator so — otherwise it copies all 128 of them before the bias add
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
                if ((mi >> 1) == half) asm volatile("" : "=v"(acc[mi][ni]));
    };

    const long long dbg_t0 = __builtin_readcyclecounter();
    // development aid (build with -DS256_TIMELINE, run with debug bit 16): wave 0 of each group stamps the cycle counter
    // at slot boundaries into LDS, dumped to out[] at the end; tools/gemm_slots.py prints the timeline.  Compiled out by
    // default: even the disabled checks cost ~5 % (everything between MFMAs does).
#ifdef S256_TIMELINE
    unsigned* sStamp = (unsigned*)(smem + 2 * S_STAGE_BYTES + p.N * 4) + grp * 1024;
    int dbg_n = 0;
    const bool dbg_on = (p.debug & 16) && blockIdx.x == 0 && wq == 0;
    auto stamp = [&]() {
        if (dbg_on && dbg_n < 1024) {
            if (lane == 0) sStamp[dbg_n] = (unsigned)(__builtin_readcyclecounter() - dbg_t0);
            ++dbg_n;
        }
    };
#else
    auto stamp = [] {};
#endif
    if (p.debug & 4) {                         // experiment: spread the CUs' tile phases over ~one tile time
        const int units = (int)(((unsigned)pid * 40503u) >> 5) & 63;
        for (int i = 0; i < units; ++i) __builtin_amdgcn_s_sleep(16);
    }
    if (p.debug & 8) {                         // experiment: one phase per XCD (L2 sharing inside an XCD is kept), spread over
        const int units = (int)(blockIdx.x & 7) * nk * ((p.debug >> 8) & 15) / 12;     // (debug>>8)&15 kilo-cycles per XCD at K=768
        for (int i = 0; i < units; ++i) __builtin_amdgcn_s_sleep(16);
    }
    if (p.bias)
        for (int i = tid; i < p.N; i += 512) sBias[i] = p.bias[i];
    __syncthreads();

    // ---- prologue: what the steady-state rules would have issued before slot 0 ----
    if (grp == 0) {
        for (int j = 0; j < 4; ++j) piece_W(0, 0, j);
        for (int j = 0; j < 4; ++j) piece_A(0, 1, j);
        S256_VMCNT(0);
    } else {
        for (int j = 0; j < 4; ++j) piece_A(0, 0, j);
        for (int j = 0; j < 4; ++j) piece_W(0, 1, j);
        if (nsteps > 1) {
            for (int j = 0; j < 4; ++j) piece_A(1, 0, j);
            for (int j = 0; j < 8; ++j) piece_W(1, j >> 2, j & 3);
            S256_VMCNT(12);
        } else {
            S256_VMCNT(0);
        }
    }
    S256_BARRIER();                                   // P: W(0) and both A-halves of step 0 are in LDS

    if (grp == 0) {
        // ================= group A =================
        for (int s = 0; s < nsteps; ++s) {
            // ---- slot 2s : R(s) ----  (a tile's first read slot starts with the second half of the previous epilogue)
            const int kt = s % nk;
            if (kt == 0 && s > 0) epilogue(s - 1, 1);
            read_step(s);
            const T256Plan q = make_plan(s);
            S256_LGKM0();
            // B's half of step s and A's half of step s+1 (issued in M(s-1)) must have landed.  Right after an
            // epilogue the 16 stores of a full tile are younger than those loads and vmcnt retires in order on gfx9, so
            // vmcnt(16) waits for the loads only and gives the stores two more slots.
            if (kt == 0 && s > 0 && stores16) S256_VMCNT(16); else S256_VMCNT(0);
            stamp();
            S256_BARRIER();
            stamp();
            // ---- slot 2s+1 : M(s) ----
            t256_mfma_step<T>(acc, wf, xf, q, kt == 0, smem_lds, vj);
            stamp();
            // Tile end.  The epilogue gets slots of its own so that it overlaps the sibling group's MFMAs instead of
            // serialising with them:   A: M(last) | E1 | E2+R(0') | M(0')      (E1 = rows 0..63 of the group's half,
            //                          B: R(last) | M(last) | E1 | E2+R(0')     E2 = rows 64..127)
            if (kt == nk - 1) { S256_BARRIER(); epilogue(s, 0); }
            S256_BARRIER();
        }
        epilogue(nsteps - 1, 1);
        S256_BARRIER();                               // matches B's last slot
    } else {
        // ================= group B (one slot behind) =================
        S256_BARRIER();                               // slot 0 (W(1) was issued in the prologue)
        for (int s = 0; s < nsteps; ++s) {
            // ---- slot 2s+1 : R(s) ----
            const int kt = s % nk;
            if (kt == 0 && s > 0) epilogue(s - 1, 1);
            read_step(s);
            const T256Plan q = make_plan(s);
            S256_LGKM0();
            if (kt == 0 && s > 0 && stores16) S256_VMCNT(16); else S256_VMCNT(0);      // the W tile of step s+1 (issued in M(s-1))
            stamp();
            S256_BARRIER();
            stamp();
            // ---- slot 2s+2 : M(s) ----
            t256_mfma_step<T>(acc, wf, xf, q, kt == 0, smem_lds, vj);
            stamp();
            if (kt == nk - 1) { S256_BARRIER(); epilogue(s, 0); }
            S256_BARRIER();
        }
        epilogue(nsteps - 1, 1);
    }
#ifdef S256_TIMELINE
    if (dbg_on && lane == 0)
        for (int i = 0; i < 1024; ++i) ((unsigned*)p.out)[8192 + grp * 1024 + i] = sStamp[i];
#endif
    // The plan is unconditional, so the last MFMA slots issued LDS-DMA loads nobody reads: they must have landed before
    // this workgroup's LDS can be handed to another workgroup.
    S256_VMCNT(0);
    if ((p.debug & 16) && tid == 0) {          // development aid: cycles and K-steps of this workgroup into out[]
        ((long long*)p.out)[2 * blockIdx.x] = __builtin_readcyclecounter() - dbg_t0;
        ((long long*)p.out)[2 * blockIdx.x + 1] = nsteps;
    }
}

template <typename T, int EPI>
int launch_epi(const Gemm16Args& a, hipStream_t s) {
    static OncePerDevice attr;
    auto kern = gemm16_s256_kernel<T, EPI>;
    const int tiles_m = (int)ceil_div(a.M, SBM), tiles_n = a.N / SBN;
    int grid;
    IISAN_TRY(t256_prepare_launch(attr, (const void*)kern, 2 * S_STAGE_BYTES + 8192 * 4, tiles_m, tiles_n, grid));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 2 * S_STAGE_BYTES + (size_t)a.N * 4 + ((a.debug & 16) ? 8192 : 0), s, a, tiles_m, tiles_n);
    IISAN_LAUNCH_OK();
    return IISAN_OK;
}

template <typename T>
int launch_t(int mode, const Gemm16Args& a, hipStream_t s) {
    switch (mode) {
        case EPI_OUT16: return launch_epi<T, EPI_OUT16>(a, s);
        case EPI_GELU16: return launch_epi<T, EPI_GELU16>(a, s);
        case EPI_QKVH16: return launch_epi<T, EPI_QKVH16>(a, s);
        default: iisan_set_error("gemm16_s256: epilogue mode %d not supported", mode); return IISAN_EBADSHAPE;
    }
}

}  // namespace

bool gemm16_s256_applicable(int mode, const Gemm16Args& a) {
    if (a.a_blk32 || a.out_blk32) return false;      // block-major intermediates: gemm16_h256 only
    return (mode == EPI_OUT16 || mode == EPI_GELU16 || mode == EPI_QKVH16) && a.N % SBN == 0 && a.N <= 8192 && a.K % SBK == 0 &&
           a.K / SBK >= 2 && (int64_t)a.lda * 2 * SBM < (1ll << 31) && (int64_t)a.ldw * 2 * SBN < (1ll << 31);
}

int launch_gemm16_s256(int dtype16, int mode, const Gemm16Args& a, hipStream_t s) {
    IISAN_CHECK_SHAPE(!a.a_blk32 && !a.out_blk32, "gemm16_s256: block-major (blk32) operands run on gemm16_h256 only");
    return dtype16 == IISAN_BF16 ? launch_t<BF16>(mode, a, s) : launch_t<F16>(mode, a, s);
}
