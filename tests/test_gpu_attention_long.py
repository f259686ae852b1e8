"""Attention past 224 tokens: the streaming-softmax kernel (the chunk walk of csrc/attn16_stream.h in the 64-wide geometry of
csrc/attn16_long.hip) behind `iisan_attention16`, the 1,024-key score row of `iisan_attention_cls16`, the `iisan_attention16_long`
primitive below the old limit and around the 16-query block and the 128-key chunk, and the routing between the kernels.

Reference, input recipe, the guarded launch and the bound 2.5 * TOL[dt] * max|ref| are those of tests/attn_stream_io.py, shared with the
80-wide geometry (tests/test_gpu_vit_huge_attention.py).  Measured values: profiles/long_sequences.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_stream_io as aio  # noqa: E402
from attn_stream_io import TOL  # noqa: E402
from iisan_amd import _lib  # noqa: E402

_stream = aio.stream


def _run(lib, entry, dt, qkvd, kbd, items, S, heads, rows):
    return aio.run(lib, entry, dt, qkvd, kbd, items, S, heads, rows).cpu().double()


def _check_both_entries(lib, dt, qkv, kb, items, S, heads, what):
    D = heads * 64
    ref = aio.attn_ref(qkv, kb, items, S, heads)
    tol = aio.bound(dt, ref)
    qkvd, kbd = aio.head_major(qkv, items, S, heads), (kb.cuda() if kb is not None else None)
    got = _run(lib, "iisan_attention16", dt, qkvd, kbd, items, S, heads, items * S)
    err = (got - ref).abs().max().item()
    got_cls = _run(lib, "iisan_attention_cls16", dt, qkvd, kbd, items, S, heads, items)
    err_cls = (got_cls - ref.view(items, S, D)[:, 0]).abs().max().item()
    print(f"{what} dt={dt}: attention16 {err:.3e} cls16 {err_cls:.3e} (bound {tol:.3e})")
    assert err <= tol, f"attention16 {what} dt={dt}: max err {err:.3e} > {tol:.3e}"
    assert err_cls <= tol, f"attention_cls16 {what} dt={dt}: max err {err_cls:.3e} > {tol:.3e}"
    return got, got_cls, ref, tol


# ---- 1. the primitive against float64 ----------------------------------------------------------------------------------------------

LONG_CASES = [(2, 225, 2, False),      # first length over the old limit
              (2, 240, 3, True),
              (1, 256, 2, True),
              (2, 257, 3, True),       # one key past a chunk / the old CLS limit
              (1, 384, 2, False),
              (2, 512, 2, True),       # BERT's ceiling
              (1, 577, 12, False),     # ViT-B/16-384
              (1, 1024, 2, False)]     # the new limit


@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("case", LONG_CASES)
def test_long_attention_vs_float64(lib, dt, case):
    items, S, heads, masked = case
    qkv, kb = aio.problem(dt, items, S, heads, masked=masked)
    _lib.dev_set("count:attn16_long", 0)
    _check_both_entries(lib, dt, qkv, kb, items, S, heads, str(case))
    assert _lib.dev_get("count:attn16_long") == 1          # iisan_attention16 ran the streaming kernel; the CLS entry has its own


# ---- 2. mask shapes the rescale can get wrong ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("S", [300, 577])
def test_long_attention_mask_shapes(lib, dt, S):
    """Item 0: keys 0..199 masked (whole chunks of uniform weights that must vanish exactly when the first real key arrives); item 1: only
    key S - 1 real; item 2: real keys only in a middle chunk (masked chunks before and behind); item 3: all masked = the mean of V."""
    items, heads = 4, 2
    qkv, _ = aio.problem(dt, items, S, heads, seed=S + 5)
    kb = torch.full((items, S), -1.0)
    kb[0, 200:] = 0.0
    kb[1, S - 1] = 0.0
    mid = 128 * ((S // 128) // 2)
    kb[2, mid:mid + 128] = 0.0
    got, got_cls, ref, tol = _check_both_entries(lib, dt, qkv, kb, items, S, heads, f"mask shapes S={S}")
    D = heads * 64
    # the single real key owns its row: V of key S - 1, rounded once
    v = qkv.double().view(items, S, 3, heads, 64)[:, :, 2].reshape(items, S, D)
    assert (got.view(items, S, D)[1] - v[1, S - 1]).abs().max().item() <= tol
    # the all-masked item: the mean of V over its S keys, for every query
    mean_v = v[3].mean(0)
    err = (got.view(items, S, D)[3] - mean_v).abs().max().item()
    err_cls = (got_cls[3] - mean_v).abs().max().item()
    print(f"all-masked S={S} dt={dt}: against mean(V) {err:.3e} cls {err_cls:.3e} (bound {tol:.3e})")
    assert err <= tol and err_cls <= tol


# ---- 3. the streaming kernel below the old limit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [0, 1])
@pytest.mark.parametrize("case", [(3, 197, 12, False), (5, 30, 12, True), (2, 224, 2, False),
                                  # around the 16-query block and around the 128-key chunk, as the 80-wide geometry is run
                                  (2, 1, 2, False), (2, 15, 2, False), (2, 16, 2, False), (1, 17, 2, False),
                                  (2, 127, 2, False), (2, 128, 2, False), (1, 129, 3, False)])
def test_long_kernel_below_the_old_limit(lib, dt, case):
    items, S, heads, masked = case
    qkv, kb = aio.problem(dt, items, S, heads, masked=masked)
    ref = aio.attn_ref(qkv, kb, items, S, heads)
    tol = aio.bound(dt, ref)
    _lib.dev_set("count:attn16_long", 0)
    got = _run(lib, "iisan_attention16_long", dt, aio.head_major(qkv, items, S, heads), kb.cuda() if kb is not None else None, items, S, heads,
               items * S)
    assert _lib.dev_get("count:attn16_long") == 1
    err = (got - ref).abs().max().item()
    print(f"attention16_long {case} dt={dt}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, f"attention16_long {case} dt={dt}: max err {err:.3e} > {tol:.3e}"


# ---- 4. routing -------------------------------------------------------------------------------------------------------------------------

def test_routing_between_the_attention_kernels(lib):
    heads = 2
    D = heads * 64
    qkvd = torch.zeros(1, heads, 3, 1025, 64, dtype=torch.float16, device="cuda")        # large enough for every S below
    ctx = torch.full((1025, D), 7.0, dtype=torch.float16, device="cuda")
    _lib.dev_set("count:attn16_long", 0)
    for S in (30, 197, 208, 224):
        _lib.check(lib.iisan_attention16(0, qkvd.data_ptr(), None, ctx.data_ptr(), 1, S, heads, _stream()), "attention16")
        assert _lib.dev_get("count:attn16_long") == 0, S
    _lib.check(lib.iisan_attention16(0, qkvd.data_ptr(), None, ctx.data_ptr(), 1, 225, heads, _stream()), "attention16")
    assert _lib.dev_get("count:attn16_long") == 1
    torch.cuda.synchronize()
    # past the limit: an error code and a message naming it, nothing launched
    ctx.fill_(7.0)
    counters = ("attn16_long", "attn16_dma")
    before = [_lib.dev_get("count:" + n) for n in counters]
    for entry in ("iisan_attention16", "iisan_attention_cls16", "iisan_attention16_long"):
        with pytest.raises(_lib.IisanHipError, match="1024"):
            _lib.check(getattr(lib, entry)(0, qkvd.data_ptr(), None, ctx.data_ptr(), 1, 1025, heads, _stream()), entry)
    torch.cuda.synchronize()
    assert [_lib.dev_get("count:" + n) for n in counters] == before
    assert (ctx == 7.0).all()
    # train-mode dropout keeps its limit
    with pytest.raises(_lib.IisanHipError):
        _lib.check(lib.iisan_attention16_dropout(0, qkvd.data_ptr(), None, ctx.data_ptr(), 1, 225, heads, 0.1, 1, 0, 0, _stream()), "S > 224")
    torch.cuda.synchronize()
    assert (ctx == 7.0).all()


# ---- 5. reproducibility at occupancy ----------------------------------------------------------------------------------------------------

def test_long_attention_at_occupancy_is_bit_reproducible_and_right(lib):
    """64 items x 12 heads x 577 tokens (ViT-B/16-384): 768 x 3 workgroups, two per CU, every chunk re-staged while other waves compute —
    twice, bit-equal (an LDS race shows up as run-to-run differences at this occupancy), and the first, a middle and the last item against
    fp32 softmax(QK^T / 8) V computed on the device."""
    items, S, heads = 64, 577, 12
    D = heads * 64
    g = torch.Generator(device="cuda").manual_seed(4)
    qkvd = (torch.randn(items, heads, 3, S, 64, device="cuda", generator=g) * 1.5).half()
    out = []
    for _ in range(2):
        ctx = torch.empty(items * S, D, dtype=torch.float16, device="cuda")
        _lib.check(lib.iisan_attention16(0, qkvd.data_ptr(), None, ctx.data_ptr(), items, S, heads, _stream()), "attention16")
        torch.cuda.synchronize()
        out.append(ctx)
    assert torch.equal(out[0], out[1])
    for it in (0, 31, 63):
        q, k, v = (qkvd[it, :, i].float() for i in range(3))                   # [H, S, 64]
        p = torch.softmax(q @ k.transpose(1, 2) / 8.0, dim=-1)
        ref = (p @ v).transpose(0, 1).reshape(S, D)
        got = out[0][it * S:(it + 1) * S].float()
        err = (got - ref).abs().max().item()
        assert err <= 2.5 * TOL[0] * ref.abs().max().item(), (it, err)
