"""`iisan_attention16_hd80` (csrc/attn16_hd80.hip): streaming-softmax attention for 80-wide heads on row-major QKV, against float64.

Reference, input recipe and bound are those of tests/test_gpu_attention_long.py: float64 softmax of the same 16-bit operands (`randn * 1.5`),
max|err| <= 2.5 * TOL[dt] * max|ref| (P and O each rounded once to 16 bits).  Shapes: around the 16-row query block (1, 15, 16, 17), around
the 128-key chunk (127, 128, 129), the tower's own 257 tokens with its 16 heads, and 577 / 1,024 (three query ranges, eight chunks).
Measured values: profiles/vit_huge.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from iisan_amd import _lib  # noqa: E402

T16 = {0: torch.float16, 1: torch.bfloat16}
TOL = {0: 2e-3, 1: 1.6e-2}       # relative to the output scale: one 16-bit rounding of the result
HD = 80


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _attn_ref(qkv, key_bias, items, S, heads):
    x = qkv.double().view(items, S, 3, heads, HD)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / (HD ** 0.5)
    if key_bias is not None:
        masked = (key_bias < 0)[:, None, None, :]
        s = torch.where(masked, torch.full_like(s, torch.finfo(torch.float32).min), s)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(items * S, heads * HD)


def _problem(dt, items, S, heads, seed=None):
    g = torch.Generator().manual_seed(S * 13 + heads if seed is None else seed)
    return (torch.randn(items * S, 3 * heads * HD, generator=g) * 1.5).to(T16[dt])


def _run(lib, dt, qkvd, kbd, items, S, heads):
    """One launch into a buffer with a guard row behind it."""
    rows, D = items * S, heads * HD
    out = torch.full((rows + 1, D), 7.0, dtype=T16[dt], device="cuda")
    _lib.check(lib.iisan_attention16_hd80(dt, qkvd.data_ptr(), kbd.data_ptr() if kbd is not None else None, out.data_ptr(), items, S, heads,
                                          _stream()), "iisan_attention16_hd80")
    torch.cuda.synchronize()
    assert (out[rows] == 7.0).all(), "attention16_hd80 wrote behind its output"
    return out[:rows]


def _check(lib, dt, qkv, kb, items, S, heads, what):
    ref = _attn_ref(qkv, kb, items, S, heads)
    tol = 2.5 * TOL[dt] * ref.abs().max().item()
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
    reference's; item 3: a mask that ends inside a chunk."""
    items, heads = 4, 2
    qkv = _problem(dt, items, S, heads, seed=S + 5)
    kb = torch.full((items, S), -1.0)
    kb[0, 128 * ((S - 1) // 128):] = 0.0
    kb[1, S - 1] = 0.0
    kb[3, :S // 2 + 3] = 0.0
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
