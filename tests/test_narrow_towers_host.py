"""Host-side logic of the narrow towers (hidden 128 - 384): the GEMM route of their ragged products and the four config constants.
No device is touched."""
from iisan_amd import _lib, weights

F16, BF16 = 0, 1
OUT16, GELU16, RESID32, PATCH32, QKVH16, PATCH16 = 0, 1, 2, 3, 4, 6
V1, S256, H256 = 0, 1, 2


def test_ragged_products_route_to_the_128x128_kernel_under_every_variant():
    """`iisan_gemm16_route` (gemm16.hip: gemm16_route): N % 128 == 64 is served by the 128x128 kernel alone — (N, K) = (192, 768) the
    patch embedding of ViT-tiny, (576, 192) its QKV, (192, 192) its O — under the auto policy and under a forced 256x256 kernel, which
    falls to it.  N % 64 != 0 is still refused, and the production shape still goes to gemm16_h256."""
    lib = _lib.load()
    M = 1_408 * 197
    for variant in (0, 3, 4):
        with _lib.dev(gemm16_variant=variant):
            for dt in (F16, BF16):
                for M_ in (3 * 197, M):
                    assert lib.iisan_gemm16_route(dt, OUT16, M_, 192, 768, 0, 0, 0, 0) == V1, (variant, dt, M_)
                    assert lib.iisan_gemm16_route(dt, PATCH16, M_, 192, 768, 196, 0, 0, 0) == V1, (variant, dt, M_)
                    assert lib.iisan_gemm16_route(dt, PATCH32, M_, 192, 768, 196, 0, 0, 0) == V1, (variant, dt, M_)
                    assert lib.iisan_gemm16_route(dt, QKVH16, M_, 576, 192, 197, 3, 0, 0) == V1, (variant, dt, M_)
                    assert lib.iisan_gemm16_route(dt, OUT16, M_, 192, 192, 0, 0, 0, 0) == V1, (variant, dt, M_)
                    assert lib.iisan_gemm16_route(dt, GELU16, M_, 192, 192, 0, 0, 0, 0) == V1, (variant, dt, M_)
                    assert lib.iisan_gemm16_route(dt, RESID32, M_, 192, 192, 0, 0, 0, 0) == V1, (variant, dt, M_)
            assert lib.iisan_gemm16_route(F16, OUT16, M, 200, 768, 0, 0, 0, 0) < 0 and b"200" in lib.iisan_last_error()
            assert lib.iisan_gemm16_route(F16, OUT16, M, 64, 768, 0, 0, 0, 0) == V1
            # LayerNorm row statistics exist on gemm16_h256 alone: never on a ragged product
            assert lib.iisan_gemm16_route(F16, QKVH16, M, 576, 192, 197, 3, 0, 1) < 0
    with _lib.dev(gemm16_variant=0):
        assert lib.iisan_gemm16_route(F16, QKVH16, 277_376, 2304, 768, 197, 12, 0, 0) == H256
    with _lib.dev(gemm16_variant=4):
        # the whole-tile products of the narrow towers still reach a forced 256x256 kernel: FC1 of ViT-tiny (K = 192: three K-steps) and of
        # BERT-tiny (K = 128: two, the shortest tile either 256x256 kernel accepts)
        assert lib.iisan_gemm16_route(F16, GELU16, 3 * 197, 768, 192, 0, 0, 0, 0) == H256
        assert lib.iisan_gemm16_route(F16, GELU16, 120, 512, 128, 0, 0, 0, 0) == H256
    with _lib.dev(gemm16_variant=3):
        assert lib.iisan_gemm16_route(F16, GELU16, 3 * 197, 768, 192, 0, 0, 0, 0) == S256


def test_narrow_tower_configs():
    for cfg, want in ((weights.VIT_TINY, (192, 12, 3, 768)), (weights.VIT_SMALL, (384, 12, 6, 1536)),
                      (weights.BERT_TINY, (128, 2, 2, 512)), (weights.BERT_MINI, (256, 4, 4, 1024))):
        assert (cfg.hidden, cfg.layers, cfg.heads, cfg.mlp) == want
        assert cfg.hidden == 64 * cfg.heads and cfg.mlp == 4 * cfg.hidden
    for cfg in (weights.BERT_TINY, weights.BERT_MINI):
        assert cfg.vocab == 30522 and cfg.eps == 1e-12 and cfg.max_pos == 512
    for cfg in (weights.VIT_TINY, weights.VIT_SMALL):
        assert cfg.tokens == 197 and cfg.patch_dim == 768 and cfg.image == 224 and cfg.patch == 16


def test_hf_converters_read_every_width_off_the_state_dict():
    """`vit_from_hf` / `bert_from_hf` carry no 768: a 192-wide / 128-wide state dict round-trips through the canonical naming."""
    import torch
    vcfg = weights.VitConfig(hidden=192, layers=2, heads=3, mlp=768, image=32, patch=16)
    bcfg = weights.BertConfig(hidden=128, layers=2, heads=2, mlp=512, vocab=64, max_pos=32)
    vw, bw = weights.make_vit_weights(vcfg, seed=3), weights.make_bert_weights(bcfg, seed=4)
    vb, bb = weights.vit_from_hf(weights.vit_to_hf5(vw, vcfg)), weights.bert_from_hf(weights.bert_to_hf(bw, bcfg))
    assert set(vb) == set(vw) and all(torch.equal(vb[k], vw[k]) for k in vw)
    assert set(bb) == set(bw) and all(torch.equal(bb[k], bw[k]) for k in bw)
    assert vb["L1.qkv_w"].shape == (576, 192) and bb["L1.fc1_w"].shape == (512, 128)
