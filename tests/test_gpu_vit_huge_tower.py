"""The frozen ViT-H/14 tower (hidden 1280 = 16 heads of 80, 14-pixel patches) through the ViT executor and every entry point, against the CPU
oracle on seeded inputs and against HuggingFace's own taps (tests/golden/vit_huge_geometry.npz).

Tolerances are the project's own (tests/test_gpu_wide_encoders.py): relative Frobenius error per tap 1.5e-3 (fp16) / 1.2e-2 (bf16), tap 0 at
1e-6 — the per-GEMM operand rounding is relative and does not depend on K, and every tower here is shallower than the 12 layers those bounds
were measured at.  Measured values: profiles/vit_huge.md."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import vit_huge_io as vio  # noqa: E402
from iisan_amd import _lib, encoders, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

TAP_TOL = {_lib.IISAN_F16: 1.5e-3, _lib.IISAN_BF16: 1.2e-2}      # relative Frobenius error per tap
TAP0 = 1e-6                                                       # tap 0: no 16-bit arithmetic on the CLS row
CLS_ONLY_TOL = 5e-4                                               # a run that stops at a shallower block against the full one
FAM = ("gemm16_h256", "gemm16_s256", "gemm16_v1")

# 17 tokens: 4 x 4 patches of 14 pixels + CLS; mlp 512 keeps the toy small, the widths that matter (1280, 16 x 80, 588 -> 640) are the tower's
TOY = weights.VitConfig(hidden=1280, layers=2, heads=16, mlp=512, image=56, patch=14)
# ViT-H/14 itself, cut to 3 layers: 257 tokens, N = 3840 / 1280 / 5120 and K = 1280 / 5120 / 640 on every GEMM family
FULL = weights.VitConfig(hidden=1280, layers=3, heads=16, mlp=5120, patch=14)
# ... and to 2 layers for the 28-image batch that reaches the production kernels
PROD = weights.VitConfig(hidden=1280, layers=2, heads=16, mlp=5120, patch=14)


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm()).item()


def _fixture(cfg, n, seed):
    vw = weights.make_vit_weights(cfg, seed=seed)
    images = vio.images(n, cfg.image, seed + 2)
    torch.set_num_threads(8)
    with torch.no_grad():
        oc = O.vit_cls_taps(images, vw, cfg)
    return SimpleNamespace(cfg=cfg, vw=vw, images=images, oc=oc, packed={})


@pytest.fixture(scope="module")
def toy():
    return _fixture(TOY, 6, seed=81)


@pytest.fixture(scope="module")
def full():
    return _fixture(FULL, 3, seed=91)


def _packed(fx, dt):
    if dt not in fx.packed:
        fx.packed[dt] = encoders.PackedVit(fx.vw, fx.cfg, "cuda", dt)
    return fx.packed[dt]


def _check_against(tc, oc, dt, what):
    assert torch.isfinite(tc).all()
    e0 = _rel(tc[:, 0], oc[:, 0])
    print(f"{what} tap 0: {e0:.3e}")
    assert e0 < TAP0, (what, e0)
    for l in range(1, oc.shape[1]):
        e = _rel(tc[:, l], oc[:, l])
        print(f"{what} tap {l}: {e:.3e} (bound {TAP_TOL[dt]:.1e})")
        assert e < TAP_TOL[dt], f"{what} tap {l}: {e:.3e}"


# ---- 1. toy tower, every entry point ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 2, 5])
@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_toy_vit_huge_matches_the_oracle(toy, dt, M):
    """Taps {0, 1, 2} of a 1280-wide 2-layer tower with 80-wide heads and 14-pixel patches, batches far below one GEMM tile, the all-zero image
    among them; a subset of taps, a chunked run and the same rows inside a larger batch return the same bits."""
    vit = _packed(toy, dt)
    img = toy.images[:M].contiguous().cuda()
    assert img[0].abs().max() == 0
    _lib.dev_set("count:attn16_hd80", 0)
    tc = vit.forward_taps(img, [0, 1, 2]).cpu()
    assert _lib.dev_get("count:attn16_hd80") == 2              # both blocks on every token: no CLS-only last block at this head width
    assert tc.shape == (M, 3, 1280)
    _check_against(tc, toy.oc[:M], dt, f"toy dt {dt} M {M}")
    assert torch.equal(vit.forward_taps(img, [0, 2]).cpu(), tc[:, [0, 2]])
    # the embedding alone: no block runs and nothing is closed (the workspace still holds the deltas of the call above)
    assert torch.equal(vit.forward_taps(img, [0]).cpu(), tc[:, [0]])
    assert torch.equal(vit.forward_taps(img, [0, 1, 2], chunk_items=3).cpu(), tc)
    assert torch.equal(vit.forward_taps(toy.images.cuda(), [0, 1, 2]).cpu()[:M], tc)


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_toy_vit_huge_with_the_fp32_residual_stream(lib, toy, dt):
    """Dev switch resid32 = 1 (`layernorm768_kernel` at width 1280 instead of the mixed kernel): the same tolerance, and really another route."""
    vit = _packed(toy, dt)
    img = toy.images[:5].contiguous().cuda()
    mc = vit.forward_taps(img, [0, 1, 2]).cpu()
    with _lib.dev(resid32=1):
        tc = vit.forward_taps(img, [0, 1, 2]).cpu()
        fc = vit.forward_taps(img, [0, 1, 2], chunk_items=2).cpu()
        t0 = vit.forward_taps(img, [0]).cpu()
        t0f = vit.forward_taps(img, [0], chunk_items=2).cpu()
    _check_against(tc, toy.oc[:5], dt, f"toy resid32 dt {dt}")
    assert torch.equal(fc, tc)
    assert torch.equal(t0, tc[:, [0]]) and torch.equal(t0f, t0)       # the embedding alone on the fp32 stream: nothing to close
    assert torch.equal(tc[:, 0], mc[:, 0]) and not torch.equal(tc, mc)


def test_toy_vit_huge_u8_and_indexed_entries_equal_the_fp32_entry(toy):
    """The u8 entry against the fp32 entry on the normalised image; the indexed entry against the direct one, an out-of-range index as the
    padding slot (the zero normalised image) — through the padded patch extraction (588 -> 640 columns)."""
    vit = _packed(toy, _lib.IISAN_F16)
    g = torch.Generator().manual_seed(7)
    u8 = torch.randint(0, 256, (5, 3, 56, 56), generator=g, dtype=torch.uint8)
    norm = (u8.float().div(255) - 0.5) / 0.5
    t_f32 = vit.forward_taps(norm.cuda(), [0, 1, 2]).cpu()
    assert torch.equal(vit.forward_taps(u8.cuda(), [0, 1, 2]).cpu(), t_f32)
    index = torch.tensor([3, 5, 0, -1, 4, 3, 99], dtype=torch.int64)                   # 5, -1, 99: outside the 5-row catalogue
    pad = (index < 0) | (index >= 5)
    direct = norm[index.clamp(0, 4)].clone()
    direct[pad] = 0
    want = vit.forward_taps(direct.cuda(), [0, 1, 2]).cpu()
    assert torch.equal(vit.forward_taps_indexed(u8.cuda(), index.cuda(), [0, 1, 2]).cpu(), want)
    assert torch.equal(vit.forward_taps_indexed(u8.cuda(), index.cuda(), [0, 1, 2], chunk_items=3).cpu(), want)
    assert not torch.equal(want[0], want[1]) and torch.isfinite(want).all()


@pytest.mark.parametrize("dt", [_lib.IISAN_F16, _lib.IISAN_BF16])
def test_vit_huge_geometry_matches_huggingface(dt):
    """The golden geometry (mlp 5120, 2 layers, 17 tokens) on the device against HuggingFace's own CLS rows, within the tap tolerance."""
    z, vw, images = vio.load_golden()
    vit = encoders.PackedVit(vw, vio.GEOM_VIT, "cuda", dt)
    tc = vit.forward_taps(images.cuda(), [0, 1, 2]).cpu()
    _check_against(tc, torch.from_numpy(z["taps"]), dt, f"HF golden dt {dt}")


# ---- 2. the full geometry through every GEMM family ---------------------------------------------------------------------------------

@pytest.fixture
def gemm_variant(lib, request):
    _lib.dev_set("gemm16_variant", request.param)
    yield request.param
    _lib.dev_set("gemm16_variant", 0)


@pytest.mark.parametrize("gemm_variant", [0, 1, 3, 4], indirect=True)
def test_full_geometry_taps_match_the_oracle_on_every_gemm_family(full, gemm_variant):
    """ViT-H/14 geometry (257 tokens, mlp 5120, 16 heads of 80, patch vector 588 -> 640) on 3 images, 3 layers, taps 0 - 3, once per GEMM kernel
    family (0 = auto, 1 = 128x128, 3 = staggered 256x256, 4 = the production 256x256 kernel); the attention is the 80-wide kernel, never the
    64-wide streaming one."""
    vit = _packed(full, _lib.IISAN_F16)
    _lib.dev_set("count:attn16_hd80", 0)
    _lib.dev_set("count:attn16_long", 0)
    tc = vit.forward_taps(full.images.cuda(), [0, 1, 2, 3]).cpu()
    assert _lib.dev_get("count:attn16_hd80") == 3 and _lib.dev_get("count:attn16_long") == 0
    _check_against(tc, full.oc, _lib.IISAN_F16, f"full variant {gemm_variant}")


def test_full_geometry_tapped_prefix_runs_fewer_blocks(lib, full):
    """Taps [0, 2] of the 3-layer tower: block 3 is dead code (counted: launches of the encoder GEMM per family); blocks 1 and 2 run on every
    token in either call, so the prefix returns the full run's bits for taps 0 and 2 and meets the tolerance."""
    vit = _packed(full, _lib.IISAN_F16)
    img = full.images.cuda()

    def launches(fn):
        for n in FAM:
            _lib.dev_set("count:" + n, 0)
        out = fn()
        return out, sum(_lib.dev_get("count:" + n) for n in FAM)

    sc, n_prefix = launches(lambda: vit.forward_taps(img, [0, 2]).cpu())
    fc, n_whole = launches(lambda: vit.forward_taps(img, [0, 1, 2, 3]).cpu())
    print(f"GEMM launches: prefix {n_prefix}, whole {n_whole}")
    assert 0 < n_prefix < n_whole, (n_prefix, n_whole)
    assert torch.equal(sc[:, 0], fc[:, 0])
    e = _rel(sc[:, 1], fc[:, 2])
    print(f"prefix [0, 2] vs full, tap 2: {e:.3e}; vs oracle {_rel(sc[:, 1], full.oc[:, 2]):.3e}")
    assert e < CLS_ONLY_TOL
    assert _rel(sc[:, 1], full.oc[:, 2]) < TAP_TOL[_lib.IISAN_F16]


# ---- 3. the production kernels ------------------------------------------------------------------------------------------------------

def test_vit_huge_reaches_the_production_kernels_at_28_images(lib):
    """28 images x 257 tokens = 29 row tiles: every 1280-column product has 29 x 5 = 145 >= 128 tiles and runs on gemm16_h256 under the auto
    dispatch (tests/test_vit_huge_host.py).  Every slot meets the tolerance; the block-major FC1 -> FC2 intermediate (blk32) is on by default —
    the counter shows it — and blk32 = 0 returns the same bits."""
    fx = _fixture(PROD, 28, seed=101)
    vit = _packed(fx, _lib.IISAN_F16)
    img = fx.images.cuda()
    out = {}
    for blk in (2, 0):
        with _lib.dev(blk32=blk):
            _lib.dev_set("count:gemm16_blk32", 0)
            _lib.dev_set("count:gemm16_h256", 0)
            out[blk] = vit.forward_taps(img, [0, 1, 2])
            torch.cuda.synchronize()
            n = _lib.dev_get("count:gemm16_blk32")
            assert _lib.dev_get("count:gemm16_h256") > 0
        assert n == (0 if blk == 0 else 2 * 2), (blk, n)            # FC1 + FC2 of 2 blocks
    assert torch.equal(out[0], out[2])
    tc = out[2].cpu()
    _check_against(tc, fx.oc, _lib.IISAN_F16, "28 images")
    for m in range(28):
        for l in (1, 2):
            e = _rel(tc[m, l], fx.oc[m, l])
            assert e < TAP_TOL[_lib.IISAN_F16], (m, l, e)
