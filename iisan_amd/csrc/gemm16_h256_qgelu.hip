// The quick-GELU (EPI_QGELU16) instantiations of the persistent 256x256 GEMM: the FC1 product of a CLIP vision tower, with a row-major
// output or with the block-major FC1 -> FC2 intermediate.  The kernel is gemm16_h256_kernel as it stands in gemm16_h256.hip — the epilogue
// mode is a template parameter there and the activation one `if constexpr` — compiled here, in a translation unit of its own, so that the
// code object of gemm16_h256.hip holds exactly the instantiations it held before the mode existed (tests/test_blk32_host.py counts them
// and holds each to its register budget; tests/test_clip_host.py does the same for the four below).
#define GEMM16_H256_KERNEL_ONLY
#include "gemm16_h256.hip"

namespace {

template <typename T>
int launch_qgelu(const Gemm16Args& a, hipStream_t s) {
    return a.out_blk32 ? launch_epi<T, EPI_QGELU16, false, BLK_OUT>(a, s) : launch_epi<T, EPI_QGELU16>(a, s);
}

}  // namespace

// gemm16_h256_applicable has turned down everything else: row statistics and a block-major A operand do not go with this mode
int launch_gemm16_h256_qgelu(int dtype16, const Gemm16Args& a, hipStream_t s) {
    IISAN_CHECK_SHAPE(!a.rowstat && !a.a_blk32, "gemm16_h256: the quick-GELU epilogue takes no row statistics and no block-major A operand");
    return dtype16 == IISAN_BF16 ? launch_qgelu<BF16>(a, s) : launch_qgelu<F16>(a, s);
}
