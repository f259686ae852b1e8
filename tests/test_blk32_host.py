"""CPU checks of the block-major ("blk32") intermediates of the persistent 256x256 GEMM: the layout formula, the
host-side route predicates, and the register budget of the changed kernel instantiations (hipcc cross-compiles gfx950)."""
import os
import re

import numpy as np
import pytest

from test_isa_screen import CSRC, _kernel_meta

H256, REJECTED = 2, -1
OUT16, GELU16, RESID32, QKVH16, PATCH16, STREAM16 = 0, 1, 2, 4, 6, 7


def blk32_byte(m, c, C):
    return ((m >> 5) * (C >> 5) + (c >> 5)) * 2048 + ((c >> 3) & 1) * 1024 + (((c >> 4) & 1) * 32 + (m & 31)) * 16 + (c & 7) * 2


def test_the_layout_is_a_bijection_and_matches_the_epilogue_lanes():
    Mp, C = 64, 96
    m, c = np.meshgrid(np.arange(Mp), np.arange(C), indexing="ij")
    byte = blk32_byte(m, c, C)
    assert sorted(byte.ravel().tolist()) == list(range(0, Mp * C * 2, 2))         # every 16-bit word of the buffer exactly once
    # a 32 x 32 block is 2 KiB contiguous, blocks row-major; lane fh * 32 + frow of the epilogue holds row frow of the block and its
    # columns 16 fh .. 16 fh + 7 in o0 (first KiB, at lane * 16) and 16 fh + 8 .. 16 fh + 15 in o1 (second KiB)
    for bm in range(Mp // 32):
        for bc in range(C // 32):
            base = (bm * (C // 32) + bc) * 2048
            for fh in range(2):
                for frow in range(32):
                    lane = fh * 32 + frow
                    for e in range(8):
                        assert blk32_byte(bm * 32 + frow, bc * 32 + 16 * fh + e, C) == base + lane * 16 + 2 * e
                        assert blk32_byte(bm * 32 + frow, bc * 32 + 16 * fh + 8 + e, C) == base + 1024 + lane * 16 + 2 * e
    # what the A-operand loader relies on: 8 rows x 64 K-elements (one 1-KiB piece of a K-step) are 8 complete 128-byte lines, and the
    # four pieces of a wave's 32 rows lie in one 4-KiB run per K-step
    K = 192
    for kt in range(K // 64):
        run = {blk32_byte(r, k, K) // 4096 for r in range(32) for k in range(kt * 64, kt * 64 + 64)}
        assert run == {kt}
        for j in range(4):
            lines = sorted({blk32_byte(8 * j + r, k, K) // 128 for r in range(8) for k in range(kt * 64, kt * 64 + 64)})
            assert len(lines) == 8
            for ln in lines:
                assert sum(1 for r in range(8) for k in range(kt * 64, kt * 64 + 64) if blk32_byte(8 * j + r, k, K) // 128 == ln) == 64


def test_route_and_applicable_predicates_carry_the_flags(lib):
    from iisan_amd import _lib
    ok = lib.iisan_gemm16_h256_applicable_blk32
    # (mode, M, N, K, S, with_rowstat, a_blk32, out_blk32)
    assert ok(GELU16, 300, 512, 128, 0, 0, 0, 1) == 1 and ok(GELU16, 300, 512, 128, 0, 1, 0, 1) == 1
    assert ok(OUT16, 300, 256, 512, 0, 0, 1, 0) == 1 and ok(STREAM16, 300, 768, 512, 5, 0, 1, 0) == 1
    assert ok(GELU16, 300, 512, 128, 0, 0, 0, 0) == 1 and ok(OUT16, 300, 256, 512, 0, 0, 0, 0) == 1
    assert ok(OUT16, 300, 256, 512, 0, 0, 0, 1) == 0        # plain output
    assert ok(GELU16, 300, 512, 128, 0, 0, 1, 0) == 0       # FC1 reading a block-major A: only the stream, under the LayerNorm epilogue ...
    assert ok(GELU16, 300, 512, 128, 0, 1, 1, 0) == 0 and ok(GELU16, 300, 512, 128, 0, 1, 1, 1) == 1      # ... and F1 block-major too
    assert ok(GELU16, 300, 512, 128, 0, 0, 1, 1) == 0 and ok(OUT16, 300, 256, 512, 0, 0, 1, 1) == 0
    assert ok(STREAM16, 300, 768, 512, 5, 0, 0, 1) == 1 and ok(STREAM16, 300, 768, 512, 5, 0, 1, 1) == 1      # the block-major stream
    assert ok(QKVH16, 300, 2304, 768, 5, 1, 1, 0) == 1      # the stream into QKV (LayerNorm epilogue) ...
    assert ok(QKVH16, 300, 2304, 768, 5, 0, 1, 0) == 0 and ok(QKVH16, 300, 2304, 768, 5, 1, 0, 1) == 0        # ... and nothing else there
    assert ok(PATCH16, 300, 768, 768, 5, 0, 1, 0) == 0 and ok(PATCH16, 300, 768, 768, 5, 0, 0, 1) == 0
    assert ok(GELU16, 300, 512 + 32, 128, 0, 0, 0, 1) == 0 and ok(OUT16, 300, 256, 512 + 32, 0, 0, 1, 0) == 0      # N % 256, K % 64
    route = lib.iisan_gemm16_route_blk32
    # (dtype16, mode, M, N, K, S, heads, which0, with_rowstat, a_blk32, out_blk32)
    try:
        for variant in (0, 1, 3):      # auto at a small shape, the 128x128 kernel, the staggered 256x256 kernel
            _lib.dev_set("gemm16_variant", variant)
            assert route(0, GELU16, 300, 512, 128, 0, 0, 0, 0, 0, 1) == REJECTED and b"blk32" in lib.iisan_last_error()
            assert route(0, OUT16, 300, 256, 512, 0, 0, 0, 0, 1, 0) == REJECTED
            assert route(0, GELU16, 300, 512, 128, 0, 0, 0, 0, 0, 0) in (0, 1)
        _lib.dev_set("gemm16_variant", 0)
        # the bench shapes take the flags under the default dispatch: ViT FC1 (LayerNorm epilogue) / FC2 (stream), BERT FC1 / FC2
        assert route(0, GELU16, 277376, 3072, 768, 0, 0, 0, 1, 0, 1) == H256 and route(0, STREAM16, 277376, 768, 3072, 197, 0, 0, 0, 1, 0) == H256
        assert route(0, GELU16, 277376, 3072, 768, 0, 0, 0, 1, 1, 1) == H256 and route(0, STREAM16, 277376, 768, 3072, 197, 0, 0, 0, 1, 1) == H256
        assert route(0, QKVH16, 277376, 2304, 768, 197, 12, 0, 1, 1, 0) == H256 and route(0, STREAM16, 277376, 768, 768, 197, 0, 0, 0, 0, 1) == H256
        assert route(0, GELU16, 42240, 3072, 768, 0, 0, 0, 0, 0, 1) == H256 and route(0, OUT16, 42240, 768, 3072, 0, 0, 0, 0, 1, 0) == H256
        assert route(1, GELU16, 42240, 3072, 768, 0, 0, 0, 0, 0, 1) == H256 and route(1, OUT16, 42240, 768, 3072, 0, 0, 0, 0, 1, 0) == H256
        _lib.dev_set("gemm16_variant", 4)
        assert route(0, GELU16, 300, 512, 128, 0, 0, 0, 0, 0, 1) == H256 and route(0, OUT16, 300, 256, 512, 0, 0, 0, 0, 1, 0) == H256
        assert route(0, OUT16, 300, 256, 512, 0, 0, 0, 0, 0, 1) == REJECTED and route(0, GELU16, 300, 512, 128, 0, 0, 0, 0, 1, 0) == REJECTED
        assert route(0, QKVH16, 300, 2304, 768, 5, 12, 0, 0, 0, 1) == REJECTED and route(0, QKVH16, 300, 2304, 768, 5, 12, 0, 0, 1, 0) == REJECTED
        assert route(0, QKVH16, 300, 2304, 768, 5, 12, 0, 1, 1, 0) == H256 and route(0, QKVH16, 300, 1536, 768, 5, 12, 1, 1, 1, 0) == H256
        assert route(0, STREAM16, 300, 768, 512, 5, 0, 0, 0, 0, 1) == H256 and route(0, STREAM16, 300, 768, 512, 5, 0, 0, 0, 1, 1) == H256
        assert route(1, GELU16, 300, 512, 128, 0, 0, 0, 1, 0, 1) == REJECTED       # LayerNorm epilogue: fp16 only
    finally:
        _lib.dev_reset()
    assert _lib.dev_get("blk32") == 2


# (vgpr_count, sgpr_spill_count) of `gemm16_h256_kernel<T, EPI, LNA>` at the parent commit 78170d5, read from the code-object metadata of
# the same command line (tests/test_isa_screen.py::_asm); both operand types gave the same figures where both exist
PARENT = {(OUT16, False): (239, 0), (GELU16, False): (248, 0), (QKVH16, False): (239, 0), (PATCH16, False): (239, 0),
          (QKVH16, True): (239, 0), (GELU16, True): (241, 2), (STREAM16, False): (243, 5)}


def test_block_major_instantiations_stay_inside_the_parents_register_budget(tmp_path):
    """Each block-major instantiation is held to the row-major instantiation it stands in for at the parent commit: no scratch, no spilled
    VGPR, VGPRs and spilled SGPRs not above the parent's.  The row-major instantiations themselves must not have moved either."""
    meta, _ = _kernel_meta(os.path.join(CSRC, "gemm16_h256.hip"), tmp_path)
    seen = {}
    for name, m in meta.items():
        k = re.search(r"gemm16_h256_kernelI(3F16|4BF16)Li(\d)ELb([01])ELi(\d)EE", name)
        if not k:
            continue
        t, epi, lna, blk = k.group(1), int(k.group(2)), k.group(3) == "1", int(k.group(4))
        seen[(t, epi, lna, blk)] = m
        vg, ss = PARENT[(epi, lna)]
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
        assert m["vgpr"] <= vg and m["sgpr_spill"] <= ss, (name, m, (vg, ss))
    # F1: FC1 out (plain, both types; LayerNorm epilogue), FC2 in (plain, both types; stream).  The ViT stream: QKV / FC1 in (LayerNorm
    # epilogue), O (stream out) and FC2 (F1 in, stream out).  Beside the eleven row-major instantiations.
    for key in [("3F16", GELU16, False, 2), ("4BF16", GELU16, False, 2), ("3F16", GELU16, True, 2), ("3F16", OUT16, False, 1),
                ("4BF16", OUT16, False, 1), ("3F16", STREAM16, False, 1), ("3F16", QKVH16, True, 1), ("3F16", GELU16, True, 3),
                ("3F16", STREAM16, False, 2), ("3F16", STREAM16, False, 3)]:
        assert key in seen, key
    assert sum(1 for k in seen if k[3] == 0) == 11 and len(seen) == 21
