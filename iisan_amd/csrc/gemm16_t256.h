// What the two persistent 256x256x64 GEMM kernels share (device code, plus the host's launch geometry at the end):
//   gemm16_s256_kernel (gemm16_s256.hip: full R | M slots, epilogue slots of their own) and
//   gemm16_h256_kernel (gemm16_h256.hip: half-slot tile boundary, LNA / stream epilogues, block-major operands).
// s256 is h256's race screen (dev switch gemm16_variant = 3): a wrong tile can be blamed on h256's boundary schedule only where
// everything else is the same code.  Here, once: tile constants, the 32x32x16 MFMA, the W-row permutation, the scheduling fences,
// the fragment reads, the DMA plan of an MFMA slot with its inline-asm piece, the full MFMA step, the persistent grid.
// Each file keeps its slot program (order of reads, waits, barriers, MFMA steps, epilogues), its tile walk and make_plan, its
// epilogues, its debug hooks and its wait macros (S256_VMCNT / S256_LGKM0: inline asm in s256, the builtin in h256 — why is written
// there).  The lane staging offsets with vj, the prologue's pieces and the accumulator / fragment-offset set-up are still written
// out in both files: moved into functions here they compile to different (not slower, but different) code, and the rule for this
// header is that both kernels' instruction streams do not change (profiles/gemm16_t256_shared.md has the instructions).
//
// The workgroup is two groups of four waves: A (grp 0; tile rows 0..127) and B (grp 1; rows 128..255), wave wq of a group owning
// the 64-column slice wq of the tile; waves w and w + 4 share a SIMD.  LDS holds a ring of two K-steps, each the A-operand tile
// (256 rows x 128 bytes) followed by the W tile.
//
// Functions here take the kernel's own arrays and scalars by reference — both kernels sit at the register limit without scratch —
// and every expression stays on the side of a scheduling fence where it is written: the LDS address of a DMA piece is summed BETWEEN
// the two fences of t256_dma_piece (formed at the call site, its two `s_add_i32` moved in front of three MFMAs of the slot).
#pragma once
#include <type_traits>

#include "common.h"

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int SBM = 256, SBN = 256, SBK = 64;
constexpr int S_OP_BYTES = SBM * SBK * 2;        // 32 KiB per operand tile
constexpr int S_STAGE_BYTES = 2 * S_OP_BYTES;    // 64 KiB per K-step

// operands are swapped in the MFMA (W rows as its "A" operand), so that a lane ends up with 16 consecutive output columns of one row
template <typename T> struct Mfma32s;
template <> struct Mfma32s<F16> {
    static __device__ __forceinline__ f16v run(h8 a, h8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct Mfma32s<BF16> {
    static __device__ __forceinline__ f16v run(b8 a, b8 b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// LDS row q of the W tile holds W row n0 + nperm32s(q).  DOCUMENTATION ONLY, no caller: the kernels write the permutation out chunk
// by chunk in their staging offsets (rowW = (16 * ((r8 >> 2) & 1) + (r8 & 3)) * ldw * 2, chunk j = W rows + 4 j: piece_W, vj, make_plan).
// Whoever changes the permutation changes it there and here.
__device__ __forceinline__ int nperm32s(int q) { return (q & ~31) + 16 * ((q >> 2) & 1) + 4 * ((q & 31) >> 3) + (q & 3); }

// The compiler must be fenced (`sched_barrier`) around every barrier / wait: MFMAs are pure register ops, and without the fences 28
// of group B's 32 MFMAs were hoisted above the `s_barrier` into its read slot and the `s_waitcnt vmcnt` to the top of the MFMA
// slot — turning the stagger back into lock-step (seen in the ISA, cost ~10 %).
#define S256_FENCE() __builtin_amdgcn_sched_barrier(0)
#define S256_BARRIER()                                   \
    do {                                                 \
        S256_FENCE();                                    \
        asm volatile("s_barrier" ::: "memory");          \
        S256_FENCE();                                    \
    } while (0)

// ---- fragment reads: LDS -> registers ----------------------------------------------------------------------------------------------
// byte offset of K-slice ks inside a 32-row run of the A tile, added to xoff: the swizzled slot, or a constant where the LDS image of
// the A operand is block-major (A_BLK, gemm16_h256 only: granule 2 ks + fh of row frow sits at
// (ks / 2) * 2048 + fh * 1024 + (ks & 1) * 512 + frow * 16)
template <bool A_BLK> __device__ __forceinline__ constexpr int t256_aslot(int ks, int slot) {
    return A_BLK ? (ks >> 1) * 2048 + (ks & 1) * 512 : slot;
}
// Fragments of flat K-step s, all four K-slices: the W fragments of the wave's slice (WITH_W) and the A-operand row blocks
// MI0 .. MI1-1 of the group's half.  <0, 4, true> is a whole read slot (24 ds_read_b128); gemm16_h256's half-steps read <0, 2, true>
// (16 reads) and <2, 4, false> (8 reads).  xoff / woff2: the lane's fragment row offsets; fh = lane >> 5, fsw = ((lane & 31) >> 1) & 7.
// Call it from a lambda of the kernel, as both files do: called at the slot sites directly, the slot of K-slice 0 comes out with
// its `v_xor_b32` operands the other way round (profiles/gemm16_t256_shared.md).
template <typename V8, int MI0, int MI1, bool WITH_W, bool A_BLK>
__device__ __forceinline__ void t256_read(const char* smem, int s, V8 (&wf)[2][4], V8 (&xf)[4][4], const int (&xoff)[4], const int (&woff2)[2],
                                          int fh, int fsw) {
    const char* sA = smem + (s & 1) * S_STAGE_BYTES;
    const char* sW = sA + S_OP_BYTES;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const int slot = ((2 * ks + fh) ^ fsw) << 4;
        if constexpr (WITH_W) {
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) wf[ni][ks] = *(const V8*)(sW + woff2[ni] + slot);
        }
#pragma unroll
        for (int mi = MI0; mi < MI1; ++mi) xf[mi][ks] = *(const V8*)(sA + xoff[mi] + t256_aslot<A_BLK>(ks, slot));
    }
}

// ---- DMA plan of one MFMA slot: 8 wave-uniform (global address, LDS offset) pairs, computed in the preceding READ
// slot (which idles ~1000 cycles at its barrier).  Nothing but the MFMAs, one 64-bit add, `s_mov m0` and the
// `global_load_lds` itself may sit in the MFMA slot: slot timelines showed every scalar instruction or branch between
// MFMAs to cost matrix-pipe time (an MFMA slot took 1440 cycles with 8 skipped `if`s, 1540 with 32, 1046 bare).
// The plan is therefore unconditional: past the end of the workgroup's steps it re-loads a valid step into
// buffers that nobody reads any more.
// Group A: pieces 0..3 = B's A-operand half of step s+1, 4..7 = A's own half of step s+2;
// group B: the W tile of step s+2 (pieces 0..3 rows 0..127, 4..7 rows 128..255).
struct T256Plan {
    uint32_t g1lo, g1hi, g2lo, g2hi;      // global byte address of pieces 0..3 / 4..7 (SGPRs)
    uint32_t l1, l2;                      // LDS byte offset of piece 0 / piece 4
};
__device__ __forceinline__ uint32_t t256_sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// One DMA piece: 1 KiB from the wave-uniform address (glo, ghi) + the lane's source offset vj_j (the kernel's vj[j]) to LDS byte
// lds_off + j KiB of the dynamic segment, whose LDS address is smem_lds.
// SGPR base + 32-bit lane offset, written as inline asm: the builtin is selected with a 64-bit VGPR address
// (a v_lshl_add_u64 per piece between the MFMAs and two address registers read per lane).  Same-box A/B
// over 6 rounds: QKV 915 -> 921, O 940 -> 942, FC1 921 -> 931, FC2 1146 -> 1162 TFLOP/s.  (M0 is only
// written here and, in the prologue, by the builtin right before its own use.)
__device__ __forceinline__ void t256_dma_piece(uint32_t smem_lds, uint32_t lds_off, int j, uint32_t vj_j, uint32_t glo, uint32_t ghi) {
    const uint64_t gb = ((uint64_t)ghi << 32) | glo;
    S256_FENCE();
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                 :: "s"(smem_lds + lds_off + j * 1024), "v"(vj_j), "s"(gb) : "memory");
    S256_FENCE();
}

// The full MFMA step: 32 MFMAs with this wave's 8 DMA pieces interleaved, piece pc after MFMA 4*pc + 3.  Only the 8 MFMAs of
// K-slice 0 exist in two versions (a tile's first K-step starts from C = 0, an inline-constant operand, instead of zeroing
// 128 VGPRs): with two full bodies the compiler hoisted the 8 piece addresses above the branch -> 16 VGPRs, spills,
// and a `s_waitcnt vmcnt(0)` for the reload at the top of every MFMA slot.
template <typename T, typename V8>
__device__ __forceinline__ void t256_mfma_step(f16v (&acc)[4][2], const V8 (&wf)[2][4], const V8 (&xf)[4][4], const T256Plan& q, bool first,
                                               uint32_t smem_lds, const uint32_t (&vj)[4]) {
    auto piece = [&](int pc) {
        const int j = pc & 3;
        t256_dma_piece(smem_lds, pc < 4 ? q.l1 : q.l2, j, vj[j], pc < 4 ? q.g1lo : q.g2lo, pc < 4 ? q.g1hi : q.g2hi);
    };
    auto slice = [&](auto FIRST, int ks) {
        f16v zero;
#pragma unroll
        for (int r = 0; r < 16; ++r) zero[r] = 0.f;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                acc[mi][ni] = Mfma32s<T>::run(wf[ni][ks], xf[mi][ks], decltype(FIRST)::value ? zero : acc[mi][ni]);
                if (((mi * 2 + ni) & 3) == 3) piece(ks * 2 + (mi >> 1));
            }
    };
    // The sibling wave of this SIMD is in its read slot (ds_reads, address VALU, plan SALU): with equal priority the
    // arbiter prefers the OLDER wave, and the slot timeline showed group B's MFMA slots at 1,680 cycles against
    // group A's 1,252.  Priority 1 for whoever is on the matrix pipe removes that.
    __builtin_amdgcn_s_setprio(1);
    if (first) slice(std::true_type{}, 0); else slice(std::false_type{}, 0);
    S256_FENCE();
#pragma unroll
    for (int ks = 1; ks < 4; ++ks) slice(std::false_type{}, ks);
    __builtin_amdgcn_s_setprio(0);
}

// ---- host: launch geometry of a persistent 256x256 kernel -------------------------------------------------------------------------
// Raises the kernel's dynamic-LDS limit once per device (`attr`: one per kernel instantiation) and returns the grid: one workgroup
// per CU (per tile where there are fewer), rounded up to whole rounds of the 8 XCDs (both tile walks take G / 8 workgroups per XCD).
inline int t256_prepare_launch(OncePerDevice& attr, const void* kern, int lds_max, int tiles_m, int tiles_n, int& grid) {
    if (attr.first())
        IISAN_HIP_OK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
    const int64_t ntiles = (int64_t)tiles_m * tiles_n;
    const int cus = iisan_cu_count();
    grid = (int)(ntiles < cus ? ntiles : cus);
    grid = (grid + 7) / 8 * 8;
    return IISAN_OK;
}
