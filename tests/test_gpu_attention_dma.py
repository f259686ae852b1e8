"""GPU tests of the LDS-DMA ViT attention kernel (csrc/attn16_dma.hip), reached through iisan_attention16.

The kernel takes the problems with no key_bias and 192 < S <= 208 (dev switch attn_route: 0 = that rule, 1 = always attention16_kernel,
2 = the DMA kernel wherever it applies).  Bound everywhere: the one of test_attention16_vs_torch, 2.5 x TOL[dt] x max|ref| (P and O are both
rounded to 16 bits)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from iisan_amd import _lib  # noqa: E402

T16 = {0: torch.float16, 1: torch.bfloat16}
TOL = {0: 2e-3, 1: 1.6e-2}       # relative to the output scale: one 16-bit rounding of the result


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _attn_ref64(qkv_hm):
    """fp64 softmax(Q K^T / 8) V of a head-major [items, heads, 3, S, 64] tensor -> [items * S, heads * 64]"""
    items, heads, _, S, _ = qkv_hm.shape
    x = qkv_hm.double().cpu()
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    p = torch.softmax(q @ k.transpose(-1, -2) / 8.0, -1)
    return (p @ v).transpose(1, 2).reshape(items * S, heads * 64)


def _attn_ref32_item(qkv_hm, it):
    q, k, v = (qkv_hm[it, :, i].float() for i in range(3))                   # [H, S, 64], on the device
    p = torch.softmax(q @ k.transpose(1, 2) / 8.0, dim=-1)
    return (p @ v).transpose(0, 1).reshape(q.shape[1], -1)


def _run(lib, dt, qkvd, ctx, kb=None):
    items, heads, _, S, _ = qkvd.shape
    _lib.check(lib.iisan_attention16(dt, qkvd.data_ptr(), kb.data_ptr() if kb is not None else None, ctx.data_ptr(), items, S, heads,
                                     _stream()), "attention16")
    torch.cuda.synchronize()


def _input(items, S, heads, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(items, heads, 3, S, 64, generator=g) * 1.5).to(T16[dt])


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("case", [(3, 197, 12), (1, 193, 2), (2, 208, 2), (2, 200, 3), (5, 197, 4)])
def test_dma_route_against_fp64(lib, dt, case):
    """The smallest S of the path, an S with no pad row, an odd head count, a single item; the default route."""
    items, S, heads = case
    qkv = _input(items, S, heads, dt, S * 13 + heads)
    ref = _attn_ref64(qkv)
    qkvd = qkv.cuda()
    ctx = torch.full((items * S, heads * 64), float("nan"), dtype=T16[dt], device="cuda")
    _lib.dev_set("count:attn16_dma", 0)
    _run(lib, dt, qkvd, ctx)
    assert _lib.dev_get("count:attn16_dma") == 1          # it IS the DMA kernel that is being checked
    err = (ctx.cpu().double() - ref).abs().max().item()
    tol = 2.5 * TOL[dt] * ref.abs().max().item()
    print(f"dma attention dt={dt} {case}: max err {err:.3e} (bound {tol:.3e})")
    assert err <= tol, f"dma attention dt={dt} {case}: max err {err:.3e} > {tol:.3e}"


@pytest.mark.parametrize("dt", [0, 1])
def test_old_route_against_new_route(lib, dt):
    """One input through attn_route 1 (attention16_kernel) and 2 (the DMA kernel): both within the bound, and within one unit in the last
    place of each other.  Observed on MI355X at this shape, fp16 and bf16: max |route 1 - route 2| = 0, not one of the 453,888 output words
    differs (profiles/attention_shared_block.md) — the transposed read delivers P·V's contraction values in the k-slots the V^T image has
    them in, and the limit, the softmax, the P rounding and the store are one piece of code for both (csrc/attn16_block.h)."""
    items, S, heads = 3, 197, 12
    qkv = _input(items, S, heads, dt, 77)
    ref = _attn_ref64(qkv)
    qkvd = qkv.cuda()
    out = {}
    try:
        for route in (1, 2):
            _lib.dev_set("attn_route", route)
            ctx = torch.full((items * S, heads * 64), float("nan"), dtype=T16[dt], device="cuda")
            _run(lib, dt, qkvd, ctx)
            out[route] = ctx.cpu().double()
    finally:
        _lib.dev_reset()
    tol = 2.5 * TOL[dt] * ref.abs().max().item()
    diff = (out[1] - out[2]).abs().max().item()
    print(f"old vs new dt={dt}: max |old - new| {diff:.3e}, old err {(out[1] - ref).abs().max().item():.3e}, "
          f"new err {(out[2] - ref).abs().max().item():.3e}, bound {tol:.3e}")
    for route in (1, 2):
        assert (out[route] - ref).abs().max().item() <= tol, route
    # Bit-equality is what is observed, not what is asserted: how the matrix cores order the fp32 sums of a 32-key and of a 16-key product is
    # not documented, and a difference there (relative 1e-7) could move an output across a rounding boundary of its 16-bit type: one unit in
    # the last place of that output, at most the unit of the largest one (2^-10 / 2^-7 relative).
    ulp = {0: 2.0 ** -10, 1: 2.0 ** -7}[dt]
    assert diff <= ulp * max(out[1].abs().max().item(), out[2].abs().max().item())


@pytest.mark.parametrize("dt", [0, 1])
def test_guard_arena(lib, dt):
    """QKV in the middle of an allocation filled with NaN, the context in the middle of one filled with a sentinel: a pad row that is not
    clamped to row S - 1 or a DMA piece that leaves its head's block brings NaN into P = 0 products; a store outside the context
    changes a sentinel."""
    items, S, heads = 2, 197, 2
    D = heads * 64
    qkv = _input(items, S, heads, dt, 5)
    ref = _attn_ref64(qkv)
    n_in, n_out, guard = qkv.numel(), items * S * D, 1 << 16
    arena_in = torch.full((n_in + 2 * guard,), float("nan"), dtype=T16[dt], device="cuda")
    arena_in[guard:guard + n_in] = qkv.cuda().reshape(-1)
    qkvd = arena_in[guard:guard + n_in].view(items, heads, 3, S, 64)
    sentinel = 12345.0 if dt == 0 else 12352.0            # exact in both types
    arena_out = torch.full((n_out + 2 * guard,), sentinel, dtype=T16[dt], device="cuda")
    ctx = arena_out[guard:guard + n_out].view(items * S, D)
    _lib.dev_set("count:attn16_dma", 0)
    _run(lib, dt, qkvd, ctx)
    assert _lib.dev_get("count:attn16_dma") == 1
    got = ctx.cpu().double()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 2.5 * TOL[dt] * ref.abs().max().item()
    assert (arena_out[:guard] == sentinel).all() and (arena_out[guard + n_out:] == sentinel).all()
    assert torch.isnan(arena_in[:guard]).all() and torch.isnan(arena_in[guard + n_in:]).all()


def test_buffer_reuse_over_more_workgroups_than_the_chip_holds(lib):
    """96 items x 12 heads = 1,152 workgroups of one head each, three to a CU: every CU runs several one after the other, and a workgroup's
    single K / V image is written by LDS-DMA into LDS the previous workgroup has just left.  Twice: bit-equal outputs (a piece that is read
    before it has landed, or a Q register taken before its load, shows as a run-to-run difference); first, middle and last item against
    fp32 on the device."""
    items, S, heads = 96, 197, 12
    D = heads * 64
    g = torch.Generator(device="cuda").manual_seed(9)
    qkvd = (torch.randn(items, heads, 3, S, 64, device="cuda", generator=g) * 1.5).half()
    out = []
    _lib.dev_set("count:attn16_dma", 0)
    for _ in range(2):
        ctx = torch.full((items * S, D), float("nan"), dtype=torch.float16, device="cuda")
        _run(lib, 0, qkvd, ctx)
        out.append(ctx)
    assert _lib.dev_get("count:attn16_dma") == 2
    assert torch.equal(out[0], out[1])
    for it in (0, 47, 95):
        ref = _attn_ref32_item(qkvd, it)
        err = (out[0][it * S:(it + 1) * S].float() - ref).abs().max().item()
        assert err <= 2.5 * TOL[0] * ref.abs().max().item(), (it, err)


def test_routing(lib):
    def launches(S, bias, items=2, heads=2):
        qkvd = _input(items, S, heads, 0, S).cuda()
        ctx = torch.empty(items * S, heads * 64, dtype=torch.float16, device="cuda")
        kb = torch.zeros(items, S, device="cuda") if bias else None
        _lib.dev_set("count:attn16_dma", 0)
        _run(lib, 0, qkvd, ctx, kb)
        return _lib.dev_get("count:attn16_dma")

    assert launches(197, False) == 1
    assert launches(30, True) == 0
    assert launches(197, True) == 0
    assert launches(224, False) == 0
    try:
        _lib.dev_set("attn_route", 1)
        assert launches(197, False) == 0
        _lib.dev_set("attn_route", 2)
        assert launches(197, False) == 1
        assert launches(197, True) == 0 and launches(224, False) == 0      # "wherever it applies"
    finally:
        _lib.dev_reset()
    assert _lib.dev_state() == ""
