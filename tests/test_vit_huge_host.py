"""ViT-H/14 (hidden 1280 = 16 heads of 80, mlp 5120, 14-pixel patches) without a device: the oracle's 80-wide-head, 14-pixel-patch
arithmetic against HuggingFace's own (`tests/golden/vit_huge_geometry.npz`), and the host-side decisions of the executors for that tower —
configuration, patch-weight padding, workspace, the kernel family of each of its five products, the encoder plan and the refusals."""
import ctypes as C

import torch

import vit_huge_io as vio
from iisan_amd import _lib, weights
from oracle import iisan_oracle as O


def test_oracle_matches_huggingface_at_the_vit_huge_geometry():
    """`oracle.vit_cls_taps` against `transformers.ViTModel` at hidden 1280 / 16 heads / mlp 5120 / patch 14 / image 56 / 2 layers: every tap within
    the project's oracle-vs-golden bound, max|err| <= 2e-5 max|ref| (tests/test_oracle_vs_golden.py).  Measured: 7.5e-7 or less per tap."""
    z, vw, images = vio.load_golden()
    torch.set_num_threads(8)
    with torch.no_grad():
        taps = O.vit_cls_taps(images, vw, vio.GEOM_VIT).double()
    ref = torch.from_numpy(z["taps"]).double()
    assert taps.shape == ref.shape == (4, 3, 1280)
    for l in range(3):
        err, scale = (taps[:, l] - ref[:, l]).abs().max().item(), ref[:, l].abs().max().item()
        print(f"oracle vs HF, tap {l}: max|err| {err:.3e} at scale {scale:.3e}")
        assert err <= 2e-5 * scale, (l, err, scale)


def test_vit_huge_config_and_padded_patch_weight():
    cfg = weights.VIT_HUGE
    assert (cfg.hidden, cfg.layers, cfg.heads, cfg.mlp, cfg.patch, cfg.image) == (1280, 32, 16, 5120, 14, 224)
    assert cfg.tokens == 257 and cfg.patch_dim == 588 and cfg.patch_ld == 640
    assert weights.VIT_BASE.patch_ld == weights.VIT_BASE.patch_dim == 768          # a multiple-of-8 patch side is not padded
    # the packed patch weight: [1280, 640], columns 588 .. 639 zero (packed on the CPU: no kernel runs in the constructor at this width)
    from iisan_amd import encoders
    toy = weights.VitConfig(hidden=1280, layers=1, heads=16, mlp=128, image=28, patch=14)
    w = weights.make_vit_weights(toy, seed=5)
    vit = encoders.PackedVit(w, toy, "cpu")
    pw = next(t for t in vit._keep if t.data_ptr() == vit.struct.patch_w)
    assert pw.shape == (1280, 640) and pw.dtype == torch.float16
    assert (pw[:, 588:] == 0).all() and torch.equal(pw[:, :588], w["patch_w"].half())
    lib = _lib.load()
    assert lib.iisan_vit_fold_bytes(C.byref(vit.struct)) == 0 and not vit.struct.folded
    assert lib.iisan_vit_forward_taps_ws_bytes(C.byref(vit.struct), 5, 0) > 0
    # the workspace of the whole tower holds the row-major QKV buffer [Tp, 3 x 1280] and the padded patch matrix beside the rest
    big = _lib.VitWeights()
    big.hidden, big.layers, big.heads, big.mlp, big.image, big.patch, big.channels = 1280, 32, 16, 5120, 224, 14, 3
    tp = -(-28 * 257 // 256) * 256
    assert lib.iisan_vit_forward_taps_ws_bytes(C.byref(big), 28, 0) >= tp * (3 * 1280 + 5120 + 4 * 1280) * 2
    assert lib.iisan_vit_forward_taps_ws_bytes(C.byref(big), 56, 28) == lib.iisan_vit_forward_taps_ws_bytes(C.byref(big), 28, 0)


def test_gemm16_routes_of_the_vit_huge_products():
    """The kernel family of the tower's five products (gemm16.hip: gemm16_route) as a literal table: 2 = gemm16_h256, 1 = gemm16_s256,
    0 = the 128x128 kernel, under gemm16_variant 0..4.  The rule (tests/test_host_logic.py): with T = ceil(M / 256) * (N / 256), variant 0 takes
    h256 where T >= 128 (half a tile per compute unit of 256); 1 and 2 force 128x128; 3 forces s256, which has no patch epilogue; 4 forces h256.
    The QKV product is a PLAIN one here (EPI_OUT16, N = 3 x 1280): the attention reads it row-major, no head-major scatter is involved.
      M = 28 x 257 = 7,196 rows = 29 row tiles:  QKV 29 x 15 = 435, O 29 x 5 = 145, FC1 29 x 20 = 580, FC2 29 x 5 = 145 — all >= 128;
                                                 patch embedding 28 x 256 = 7,168 rows = 28 tiles x 5 = 140 >= 128;
      M = 3 x 257 = 771 rows = 4 row tiles:      60, 20, 80, 20, and 768 patch rows = 3 tiles x 5 = 15 — all < 128: auto stays on 128x128.
    Both operand types route alike (none of these products has LayerNorm or a residual add in its epilogue at this width).  The routes depend
    on the shapes alone, so this table also holds on the code before the tower; it pins what the GPU tests of the tower rely on."""
    lib = _lib.load()
    OUT16, GELU16, PATCH16 = 0, 1, 6
    # (mode, M, N, K, P for PATCH16) -> route under variants 0..4
    table = [
        ((OUT16, 7196, 3840, 1280, 0), (2, 0, 0, 1, 2)),           # 28 images: QKV, T = 435
        ((OUT16, 7196, 1280, 1280, 0), (2, 0, 0, 1, 2)),           # O, T = 145
        ((GELU16, 7196, 5120, 1280, 0), (2, 0, 0, 1, 2)),          # FC1, T = 580
        ((OUT16, 7196, 1280, 5120, 0), (2, 0, 0, 1, 2)),           # FC2, T = 145
        ((PATCH16, 7168, 1280, 640, 256), (2, 0, 0, 0, 2)),        # patch embedding over the padded K = 640, T = 140; no s256 patch epilogue
        ((OUT16, 771, 3840, 1280, 0), (0, 0, 0, 1, 2)),            # 3 images: QKV, T = 60
        ((OUT16, 771, 1280, 1280, 0), (0, 0, 0, 1, 2)),            # O, T = 20
        ((GELU16, 771, 5120, 1280, 0), (0, 0, 0, 1, 2)),           # FC1, T = 80
        ((OUT16, 771, 1280, 5120, 0), (0, 0, 0, 1, 2)),            # FC2, T = 20
        ((PATCH16, 768, 1280, 640, 256), (0, 0, 0, 0, 2)),         # patch embedding, T = 15
    ]
    for variant in range(5):
        with _lib.dev(gemm16_variant=variant):
            for dt in (0, 1):
                for (mode, M, N, K, S), want in table:
                    got = lib.iisan_gemm16_route(dt, mode, M, N, K, S, 0, 0, 0)
                    assert got == want[variant], (variant, dt, mode, M, N, K, got, want[variant])


def test_encoder_plan_of_the_vit_huge_tower_and_its_refusals():
    """`iisan_encoder_plan` for hidden 1280 / 16 heads: bit 32 (row-major QKV, attn16_hd80, the last live block on every token) on the
    LayerNorm-image route (1) whatever ln_fold says, with the block-major FC1 -> FC2 intermediate (4) once FC1 and FC2 reach gemm16_h256;
    resid32 = 1 gives the fp32 stream (0).  1280 with 20 heads, and 1280 on the BERT executor, stay refused with today's wording."""
    lib = _lib.load()
    VIT, BERT = 0, 1
    huge = lambda dt=0, M=1408, heads=16, tower=VIT, tokens=257, full=0: (tower, dt, 1280, heads, 5120, tokens, M, 0, 32, full, 0)
    for dt in (0, 1):
        assert lib.iisan_encoder_plan(*huge(dt)) == 32 | 4 | 1
        assert lib.iisan_encoder_plan(*huge(dt, M=4)) == 32 | 1                      # 4 x 257 rows: the products stay on 128x128, F1 row-major
        assert lib.iisan_encoder_plan(*huge(dt, full=1)) == 32 | 4 | 1
        for ln_fold in (0, 1, 2):
            with _lib.dev(ln_fold=ln_fold):
                assert lib.iisan_encoder_plan(*huge(dt)) == 32 | 4 | 1
        with _lib.dev(blk32=0):
            assert lib.iisan_encoder_plan(*huge(dt)) == 32 | 1
        with _lib.dev(resid32=1):
            assert lib.iisan_encoder_plan(*huge(dt)) & 3 == 0 and lib.iisan_encoder_plan(*huge(dt)) & 32
    assert lib.iisan_encoder_plan(*huge(tokens=1025)) < 0
    import re
    for case in (huge(heads=20), huge(tower=BERT, tokens=30), huge(tower=BERT, heads=20, tokens=30)):
        assert lib.iisan_encoder_plan(*case) < 0, case
        assert re.search("768.*1024", lib.iisan_last_error().decode()), lib.iisan_last_error()
    # every width that ran before answers as before: no bit 32
    assert lib.iisan_encoder_plan(VIT, 0, 1024, 16, 4096, 197, 1408, 0, 24, 0, 1) & 32 == 0
    assert "iisan_attention16_hd80" in _lib.SIGNATURES
