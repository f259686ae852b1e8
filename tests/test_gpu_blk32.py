"""GPU tests of the block-major ("blk32") intermediates of the persistent 256x256 GEMM (`csrc/gemm16_h256.hip`).

The layout changes where bytes go, never arithmetic or summation order: every comparison here is BIT-EQUALITY of raw 16-bit words against
the row-major route of the same kernel (forced with `gemm16_variant = 4`), after de-blocking on the host with the formula written out
below — the library is not asked for it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402
from iisan_amd import _lib, encoders, weights  # noqa: E402

T16 = {0: torch.float16, 1: torch.bfloat16}
NAN16 = {0: 0x7E00, 1: 0x7FC0}        # a quiet-NaN bit pattern of either 16-bit type
EBADSHAPE = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def blk32_index(Mp, C, device="cuda"):
    """[Mp, C] -> index of element (m, c) in 16-bit words of the block-major matrix: byte
    ((m >> 5) * (C >> 5) + (c >> 5)) * 2048 + ((c >> 3) & 1) * 1024 + (((c >> 4) & 1) * 32 + (m & 31)) * 16 + (c & 7) * 2"""
    m = torch.arange(Mp, device=device)[:, None]
    c = torch.arange(C, device=device)[None, :]
    byte = ((m >> 5) * (C >> 5) + (c >> 5)) * 2048 + ((c >> 3) & 1) * 1024 + (((c >> 4) & 1) * 32 + (m & 31)) * 16 + (c & 7) * 2
    return byte >> 1


def deblock(buf, Mp, C):
    """raw words (int16) of a block-major [Mp, C] buffer -> row-major [Mp, C]"""
    return buf.view(torch.int16).reshape(-1)[blk32_index(Mp, C, buf.device)]


def block(t):
    """row-major [Mp, C] 16-bit tensor -> the same elements block-major"""
    Mp, C = t.shape
    out = torch.empty(Mp * C, dtype=torch.int16, device=t.device)
    out[blk32_index(Mp, C, t.device).reshape(-1)] = t.view(torch.int16).reshape(-1)
    return out.view(t.dtype).reshape(Mp, C)


def _nan_filled(rows, cols, dt):
    return torch.full((rows, cols), NAN16[dt], dtype=torch.int16, device="cuda").view(T16[dt])


def _chain_case(M, N1, dt, lna):
    K1, N2 = 128, 256
    Mp = (M + 255) // 256 * 256
    g = torch.Generator(device="cuda").manual_seed(M + N1 + 7 * dt + lna)
    x = torch.zeros(Mp, K1, dtype=T16[dt], device="cuda")
    x[:M] = (torch.randn(M, K1, generator=g, device="cuda") * 0.5).to(T16[dt])
    W1 = (torch.randn(N1, K1, generator=g, device="cuda") * 0.1).to(T16[dt])
    b1 = torch.randn(N1, generator=g, device="cuda") * 0.3
    W2 = (torch.randn(N2, N1, generator=g, device="cuda") * 0.05).to(T16[dt])
    b2 = torch.randn(N2, generator=g, device="cuda") * 0.3
    rstat = (torch.rand(Mp, generator=g, device="cuda") + 0.5) if lna else None
    return Mp, K1, N2, x, W1, b1, W2, b2, rstat


@pytest.mark.parametrize("M,N1", [(256, 512), (300, 512), (2088, 1024)])
@pytest.mark.parametrize("dt,lna", [(0, False), (1, False), (0, True)])
def test_fc1_fc2_chain_block_major_is_bit_equal_to_row_major(lib, M, N1, dt, lna):
    """x [M, 128] -> F1 = GELU(x W1^T + b1) (N1 wide, K = 128: two K-steps, the minimum; `lna`: one rstd per row applied in the epilogue)
    -> out = F1 W2^T + b2 (256 wide).  M = 256: one full tile; 300: a ragged second tile whose last block row (288..319) is partial;
    2,088 x 1,024: nine row tiles and four column tiles under a panel walk of three.  The blocked F1 starts as NaN patterns everywhere:
    its rows < M must equal the row-major F1 word for word, its pad rows must stay untouched, and no NaN may reach an output row < M."""
    Mp, K1, N2, x, W1, b1, W2, b2, rstat = _chain_case(M, N1, dt, lna)
    rs = rstat.data_ptr() if lna else None
    res = {}
    try:
        _lib.dev_set("gemm16_variant", 4)
        if M > 2048:
            (_lib.dev_set("gemm16_walk_c", 3), _lib.dev_set("gemm16_walk_h", 2))
        for blk in (0, 1):
            F1 = _nan_filled(Mp, N1, dt)
            out = _nan_filled(Mp, N2, dt)
            _lib.check(lib.iisan_gemm16_blk32(dt, 1, x.data_ptr(), W1.data_ptr(), b1.data_ptr(), F1.data_ptr(), rs, M, N1, K1, 0, blk, _stream()), "FC1")
            _lib.check(lib.iisan_gemm16_blk32(dt, 0, F1.data_ptr(), W2.data_ptr(), b2.data_ptr(), out.data_ptr(), None, M, N2, N1, blk, 0, _stream()), "FC2")
            res[blk] = (F1, out)
        assert _lib.dev_get("count:gemm16_blk32") == 2
        if lna:     # the stream into FC1: a block-major A operand under the LayerNorm epilogue (rstd per row), F1 block-major
            F1x = _nan_filled(Mp, N1, dt)
            _lib.check(lib.iisan_gemm16_blk32(dt, 1, block(x).data_ptr(), W1.data_ptr(), b1.data_ptr(), F1x.data_ptr(), rs, M, N1, K1, 1, 1, _stream()), "FC1, A block-major")
    finally:
        _lib.dev_reset()
    torch.cuda.synchronize()
    F1_rm, out_rm = (t.view(torch.int16) for t in res[0])
    F1_bm, out_bm = deblock(res[1][0], Mp, N1), res[1][1].view(torch.int16)
    assert torch.isfinite(res[0][0][:M].float()).all() and torch.isfinite(res[0][1][:M].float()).all()
    assert torch.equal(F1_bm[:M], F1_rm[:M])
    nan = NAN16[dt]
    assert (F1_bm[M:] == nan).all() and (F1_rm[M:] == nan).all()        # pad rows: never written, in either layout
    assert not torch.equal(res[1][0].view(torch.int16)[:M], F1_rm[:M])   # (the blocked buffer really is laid out differently)
    assert torch.equal(out_bm[:M], out_rm[:M])
    assert (out_bm[M:] == nan).all()
    if lna:
        assert torch.equal(F1x.view(torch.int16), res[1][0].view(torch.int16))


@pytest.mark.parametrize("M", [300, 2088])
def test_stream_product_reads_a_block_major_a_operand(lib, M):
    """The FC2 product of the product route adds into the fp16 stream (`EPI_STREAM16`) and reads F1: with F1 block-major, the stream
    (N = 768), the per-slice row sums and what `stream_stats_finalize` makes of them must be bit-equal to the row-major chain.  S = 5:
    CLS rows fall inside tiles."""
    S, N, N1, K1 = 5, 768, 512, 128
    items = (M + S - 1) // S
    Mp, _, _, x, W1, b1, _, _, _ = _chain_case(M, N1, 0, False)
    g = torch.Generator(device="cuda").manual_seed(M)
    W2 = (torch.randn(N, N1, generator=g, device="cuda") * 0.05).half()
    b2 = torch.randn(N, generator=g, device="cuda") * 0.3
    x0 = torch.zeros(Mp, N, dtype=torch.float16, device="cuda")
    x0[:M] = (torch.randn(M, N, generator=g, device="cuda") * 1.5 + 0.2).half()
    xc0 = torch.randn(items, N, generator=g, device="cuda") * 1.5
    runs = {}
    try:
        _lib.dev_set("gemm16_variant", 4)
        for blk in (0, 1):
            F1 = _nan_filled(Mp, N1, 0)
            xs, xc = x0.clone(), xc0.clone()
            part = torch.zeros(N // 64, Mp, 2, device="cuda"); rstd = torch.zeros(Mp, device="cuda")
            _lib.check(lib.iisan_gemm16_blk32(0, 1, x.data_ptr(), W1.data_ptr(), b1.data_ptr(), F1.data_ptr(), None, M, N1, K1, 0, blk, _stream()), "FC1")
            _lib.check(lib.iisan_gemm16_stream_blk32(F1.data_ptr(), W2.data_ptr(), b2.data_ptr(), xs.data_ptr(), part.data_ptr(), M, N, N1, S, blk, 0, _stream()), "FC2")
            xg = xs.clone()
            # (M need not be a multiple of S here: the finalize step takes the whole items only)
            _lib.check(lib.iisan_stream_stats_finalize(part.data_ptr(), N // 64, Mp, xs.data_ptr(), xc.data_ptr(), rstd.data_ptr(), 1e-6, M // S, S, _stream()), "finalize")
            runs[blk] = (xg, part[:, :M].clone(), xs, xc, rstd[:M // S * S].clone())
    finally:
        _lib.dev_reset()
    torch.cuda.synchronize()
    assert torch.isfinite(runs[0][0][:M].float()).all() and not torch.equal(runs[0][0], x0)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.float16 else a, b.view(torch.int16) if b.dtype == torch.float16 else b)


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M", [300, 2088])
def test_stream_product_on_a_block_major_stream(lib, M, K):
    """`EPI_STREAM16` with the stream x16 [Mp, 768] block-major (the O form: A row-major; the FC2 form: A block-major too), S = 5 so
    that CLS rows fall inside tiles; K = 128 / 256: two / four K-steps.  x16 (de-blocked) and the row sums must be bit-equal to the
    row-major form; then `stream_stats_finalize`: rstd, the fp32 CLS stream and the rewritten CLS rows as well."""
    S, N = 5, 768
    items = M // S
    Mp = (M + 255) // 256 * 256
    g = torch.Generator(device="cuda").manual_seed(M + K)
    A = torch.zeros(Mp, K, dtype=torch.float16, device="cuda")
    A[:M] = (torch.randn(M, K, generator=g, device="cuda") * 0.5).half()
    W = (torch.randn(N, K, generator=g, device="cuda") * 0.05).half()
    b = torch.randn(N, generator=g, device="cuda") * 0.3
    x0 = torch.zeros(Mp, N, dtype=torch.float16, device="cuda")
    x0[:M] = (torch.randn(M, N, generator=g, device="cuda") * 1.5 + 0.2).half()
    xc0 = torch.randn(items, N, generator=g, device="cuda") * 1.5
    runs = {}
    try:
        _lib.dev_set("gemm16_variant", 4)
        for a_blk, x_blk in ((0, 0), (0, 1), (1, 1)):
            Ad = block(A) if a_blk else A
            xs = block(x0) if x_blk else x0.clone()
            xc = xc0.clone()
            part = torch.zeros(N // 64, Mp, 2, device="cuda"); rstd = torch.zeros(Mp, device="cuda")
            _lib.check(lib.iisan_gemm16_stream_blk32(Ad.data_ptr(), W.data_ptr(), b.data_ptr(), xs.data_ptr(), part.data_ptr(), M, N, K, S, a_blk, x_blk, _stream()), "stream")
            xg = xs.clone()
            _lib.check(lib.iisan_stream_stats_finalize_blk32(part.data_ptr(), N // 64, Mp, xs.data_ptr(), xc.data_ptr(), rstd.data_ptr(), 1e-6, items, S, x_blk, _stream()), "finalize")
            de = (lambda t: deblock(t, Mp, N)) if x_blk else (lambda t: t.view(torch.int16))
            runs[(a_blk, x_blk)] = (de(xg), part[:, :M].clone(), de(xs), xc, rstd[:items * S].clone())
    finally:
        _lib.dev_reset()
    torch.cuda.synchronize()
    ref = runs[(0, 0)]
    assert torch.isfinite(ref[0][:M].view(torch.float16).float()).all() and not torch.equal(ref[0], x0.view(torch.int16))
    assert not torch.equal(ref[0], ref[2])                      # (the finalize step rewrote the CLS rows)
    for key in ((0, 1), (1, 1)):
        for a, b2 in zip(ref, runs[key]):
            assert torch.equal(a, b2), key


def _tower_inputs(items):
    g = torch.Generator().manual_seed(5)
    images = torch.randn(items, 3, gio.E2E_VIT.image, gio.E2E_VIT.image, generator=g)
    words = 8
    ids = torch.randint(1, gio.E2E_BERT.vocab, (items, words), generator=g)
    mask = (torch.arange(words)[None, :] < torch.randint(2, words + 1, (items, 1), generator=g)).long()
    return images.cuda(), torch.cat([ids * mask, mask], 1).contiguous().cuda()


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_towers_give_the_same_taps_at_every_blk32_level(lib, dt):
    """Both towers (two blocks at hidden 768) on 70 items — 350 / 560 token rows, two / three row tiles with a ragged last one — with
    the production kernel forced: the taps under `blk32 = 0`, under 1 (F1 block-major) and under 2 (the default: the ViT stream as well)
    must be equal, for the whole batch and for chunks of 32 (last chunk: 6 items), with every block on every token and with the
    CLS-only last block.  fp16: the ViT executor takes the stream route (LayerNorm in the QKV / FC1 epilogues, O / FC2 add into the
    stream); bf16: LayerNorm images and plain FC1 / FC2 products.  The launch counter shows that each level really ran its block-major
    products and that the switch really turned them off."""
    items = 70
    images, text = _tower_inputs(items)
    vit = encoders.PackedVit(weights.make_vit_weights(gio.E2E_VIT, seed=11), gio.E2E_VIT, "cuda", dt)
    bert = encoders.PackedBert(weights.make_bert_weights(gio.E2E_BERT, seed=12), gio.E2E_BERT, "cuda", dt)
    layers = [0, 1, 2]
    taps, counts = {}, {}
    assert _lib.dev_get("blk32") == 2
    try:
        for blk in (0, 1, 2):
            for fb in (0, 1):
                for chunk in (0, 32):
                    _lib.dev_reset()
                    _lib.dev_set("gemm16_variant", 4)
                    _lib.dev_set("full_blocks", fb)
                    _lib.dev_set("blk32", blk)
                    taps[(blk, fb, chunk)] = (vit.forward_taps(images, layers, chunk_items=chunk), bert.forward_taps(text, layers, chunk_items=chunk))
                    counts[(blk, fb, chunk)] = _lib.dev_get("count:gemm16_blk32")
    finally:
        _lib.dev_reset()
    torch.cuda.synchronize()
    for fb in (0, 1):
        for chunk in (0, 32):
            for blk in (1, 2):
                for t0, t1 in zip(taps[(0, fb, chunk)], taps[(blk, fb, chunk)]):
                    assert torch.isfinite(t0).all() and torch.equal(t0, t1), (blk, fb, chunk)
            assert counts[(0, fb, chunk)] == 0
            # level 1: FC1 + FC2 of every all-token block, both towers, every chunk: 1 block (CLS-only last block) or 2.  Level 2, the
            # ViT's stream route (fp16): QKV, O, FC1, FC2 of every all-token block + the K/V product of a CLS-only last block
            chunks, blocks = (3 if chunk else 1), 1 + fb
            assert counts[(1, fb, chunk)] == chunks * blocks * (2 + 2), (fb, chunk, counts[(1, fb, chunk)])
            vit2 = blocks * 4 + (1 - fb) if dt == _lib.IISAN_F16 else blocks * 2
            assert counts[(2, fb, chunk)] == chunks * (vit2 + blocks * 2), (fb, chunk, counts[(2, fb, chunk)])


def test_the_flags_are_rejected_wherever_no_kernel_carries_them(lib):
    """A block-major buffer read or written row-major would be silent garbage: every other kernel route and every epilogue mode that does
    not carry a flag must turn it down with IISAN_EBADSHAPE."""
    M, N, K = 512, 512, 256
    A = torch.zeros(M, K, dtype=torch.float16, device="cuda")
    W = torch.zeros(N, K, dtype=torch.float16, device="cuda")
    b = torch.zeros(N, device="cuda")
    out = torch.zeros(M, N, dtype=torch.float16, device="cuda")
    part = torch.zeros(N // 64, M, 2, device="cuda")
    rs = torch.ones(M, device="cuda")

    def gemm(dt, mode, a_blk, o_blk, rowstat=None):
        return lib.iisan_gemm16_blk32(dt, mode, A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), rowstat, M, N, K, a_blk, o_blk, _stream())

    def stream(a_blk, x_blk):
        return lib.iisan_gemm16_stream_blk32(A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), part.data_ptr(), M, N, K, 5, a_blk, x_blk, _stream())

    try:
        for variant in (0, 1, 3):          # auto (a shape this small runs on the 128x128 kernel), 128x128 forced, the staggered 256x256 kernel
            _lib.dev_set("gemm16_variant", variant)
            assert gemm(0, 1, 0, 1) == EBADSHAPE and b"blk32" in lib.iisan_last_error()
            assert gemm(0, 0, 1, 0) == EBADSHAPE
            assert gemm(0, 0, 0, 0) == 0 and gemm(0, 1, 0, 0) == 0          # (the same calls without a flag run)
        _lib.dev_set("gemm16_variant", 4)
        for dt in (0, 1):
            assert gemm(dt, 0, 0, 1) == EBADSHAPE       # plain output: no block-major epilogue
            assert gemm(dt, 1, 1, 0) == EBADSHAPE       # FC1 reading a block-major A: only the stream, under the LayerNorm epilogue
            assert gemm(dt, 0, 1, 1) == EBADSHAPE and gemm(dt, 1, 1, 1) == EBADSHAPE
            assert gemm(dt, 1, 0, 1) == 0 and gemm(dt, 0, 1, 0) == 0
        assert gemm(1, 1, 0, 1, rs.data_ptr()) == EBADSHAPE                 # LayerNorm in the epilogue: fp16 only, with or without the flag
        assert gemm(0, 1, 0, 1, rs.data_ptr()) == 0 and gemm(0, 1, 1, 1, rs.data_ptr()) == 0
        assert gemm(0, 1, 1, 0, rs.data_ptr()) == EBADSHAPE                 # ... and FC1 then writes F1 block-major too
        assert gemm(0, 0, 1, 0, rs.data_ptr()) == EBADSHAPE                 # no LayerNorm epilogue on the plain product
        for a_blk, x_blk in ((0, 0), (1, 0), (0, 1), (1, 1)):
            assert stream(a_blk, x_blk) == 0
        assert lib.iisan_gemm16_blk32(0, 4, A.data_ptr(), W.data_ptr(), b.data_ptr(), out.data_ptr(), None, M, N, K, 0, 1, _stream()) == EBADSHAPE
    finally:
        _lib.dev_reset()
    torch.cuda.synchronize()
