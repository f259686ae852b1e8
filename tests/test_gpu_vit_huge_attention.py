"""`iisan_attention16_hd80`: streaming-softmax attention for 80-wide heads on row-major QKV (the chunk walk of csrc/attn16_stream.h in the
geometry of csrc/attn16_hd80.hip), against float64.

Reference, input recipe, the guarded launch and the bound 2.5 * TOL[dt] * max|ref| are those of tests/attn_stream_io.py, shared with the
64-wide geometry (tests/test_gpu_attention_long.py).  Shapes: around the 16-row query block (1, 15, 16, 17), around the 128-key chunk
(127, 128, 129), the tower's own 257 tokens with its 16 heads, and 577 / 1,024 (three query ranges, eight chunks).
Measured values: profiles/vit_huge.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_stream_io as aio  # noqa: E402
from iisan_amd import _lib  # noqa: E402

HD = 80
_stream = aio.stream


def _problem(dt, items, S, heads, seed=None):
    return aio.problem(dt, items, S, heads, HD, seed=seed)[0]


def _run(lib, dt, qkvd, kbd, items, S, heads):
    return aio.run(lib, "iisan_attention16_hd80", dt, qkvd, kbd, items, S, heads, items * S, HD)


def _check(lib, dt, qkv, kb, items, S, heads, what):
    ref = aio.attn_ref(qkv, kb, items, S, heads, HD)
    tol = aio.bound(dt, ref)
    got = _run(lib, dt, qkv.cuda(), kb.cuda() if kb is not None else None, items, S, heads).cpu().double()
    err = (got - ref).abs().max().item()
    print(f"attention16_hd80 {what} dt={dt}: max err {err:.3e} (bound {tol:.3e})")
    assert torch.isfinite(got).all()
    assert err <= tol, f"attention16_hd80 {what} dt={dt}: max err {err:.3e} > {tol:.3e}"
    return got, ref, tol


CASES = [(2, 1, 2), (2, 15, 2), (2, 16, 2), (1, 17, 16),         # (items, S, heads): around the 16-row block
         (2, 127, 2), (2, 128, 2), (1, 129, 3),                  # around the 128-key chunk
         (1, 257, 16),                                           # ViT-H/14 at 224 pixels
         (1, 577, 2), (1, 1024, 2)]


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("case", CASES)
def test_hd80_attention_vs_float64(lib, dt, case):
    items, S, heads = case
    _lib.dev_set("count:attn16_hd80", 0)
    _lib.dev_set("count:attn16_long", 0)
    _check(lib, dt, _problem(dt, items, S, heads), None, items, S, heads, str(case))
    assert _lib.dev_get("count:attn16_hd80") == 1 and _lib.dev_get("count:attn16_long") == 0


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("S", [129, 300])
def test_hd80_attention_mask_shapes(lib, dt, S):
    """Item 0: a masked prefix spanning whole chunks (keys 0 .. 127 at S = 129, 0 .. 255 at S = 300: uniform weights that must vanish exactly
    when the first real key arrives); item 1: only the last key real — its row is V of that key; item 2: all masked — every chunk keeps the
    running maximum at MASK_RAW c2, the rescale factor between chunks is exp2(0) = 1, and the row is softmax of equal scores like the
    reference's; item 3: a mask that ends inside a chunk; item 4: real keys only in one middle chunk (masked chunks before and behind)."""
    items, heads = 5, 2
    qkv = _problem(dt, items, S, heads, seed=S + 5)
    kb = torch.full((items, S), -1.0)
    kb[0, 128 * ((S - 1) // 128):] = 0.0
    kb[1, S - 1] = 0.0
    kb[3, :S // 2 + 3] = 0.0
    mid = 128 * ((S // 128) // 2)
    kb[4, mid:mid + 128] = 0.0
    got, ref, tol = _check(lib, dt, qkv, kb, items, S, heads, f"mask shapes S={S}")
    D = heads * HD
    v = qkv.double().view(items, S, 3, heads, HD)[:, :, 2].reshape(items, S, D)
    assert (got.view(items, S, D)[1] - v[1, S - 1]).abs().max().item() <= tol
    err = (got.view(items, S, D)[2] - ref.view(items, S, D)[2]).abs().max().item()
    print(f"all-masked item S={S} dt={dt}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol


def test_hd80_attention_is_bit_reproducible(lib):
    """The tower's shape, 8 items x 16 heads x 257 tokens = 256 workgroups re-staging chunks while others compute: two launches, equal bits
    (an LDS race shows up as run-to-run differences)."""
    items, S, heads = 8, 257, 16
    qkvd = _problem(0, items, S, heads, seed=3).cuda()
    a, b = _run(lib, 0, qkvd, None, items, S, heads), _run(lib, 0, qkvd, None, items, S, heads)
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()


def test_hd80_attention_refuses_more_than_1024_tokens(lib):
    heads = 2
    qkvd = torch.zeros(1025, 3 * heads * HD, dtype=torch.float16, device="cuda")
    ctx = torch.full((1025, heads * HD), 7.0, dtype=torch.float16, device="cuda")
    before = _lib.dev_get("count:attn16_hd80")
    with pytest.raises(_lib.IisanHipError, match="1024"):
        _lib.check(lib.iisan_attention16_hd80(0, qkvd.data_ptr(), None, ctx.data_ptr(), 1, 1025, heads, _stream()), "S = 1025")
    torch.cuda.synchronize()
    assert _lib.dev_get("count:attn16_hd80") == before and (ctx == 7.0).all()
