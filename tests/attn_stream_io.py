"""Shared pieces of the streaming-softmax attention tests (tests/test_gpu_attention_long.py: 64-wide heads, head-major input;
tests/test_gpu_vit_huge_attention.py: 80-wide heads, row-major input): the float64 reference, the seeded problem, the head-major
permutation and the guarded launch, by head width.

Reference and input recipe are those of tests/test_gpu_primitives.py::test_attention16_vs_torch: float64 softmax of the same 16-bit
operands, `randn * 1.5`.  The bound both files hold the kernels to is 2.5 * TOL[dt] * max|ref|: P and O are each rounded once to 16 bits,
and the fp32 rescale of the running sum and context adds nothing at that scale."""
import torch

from iisan_amd import _lib

T16 = {0: torch.float16, 1: torch.bfloat16}
TOL = {0: 2e-3, 1: 1.6e-2}       # relative to the output scale: one 16-bit rounding of the result


def stream():
    return torch.cuda.current_stream().cuda_stream


def bound(dt, ref):
    return 2.5 * TOL[dt] * ref.abs().max().item()     # P and O are both rounded to 16 bit


def attn_ref(qkv, key_bias, items, S, heads, hd=64):
    """float64 softmax(Q K^T / sqrt(hd) + mask) V of row-major qkv [items * S, 3 * heads * hd]; [items * S, heads * hd]"""
    x = qkv.double().view(items, S, 3, heads, hd)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) / (hd ** 0.5)
    if key_bias is not None:
        masked = (key_bias < 0)[:, None, None, :]
        s = torch.where(masked, torch.full_like(s, torch.finfo(torch.float32).min), s)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(items * S, heads * hd)


def problem(dt, items, S, heads, hd=64, masked=False, seed=None):
    """(qkv, key_bias): row-major `randn * 1.5` in the 16-bit type; masked = every item keeps a random number of leading keys, item 0 none"""
    g = torch.Generator().manual_seed(S * 13 + heads if seed is None else seed)
    qkv = (torch.randn(items * S, 3 * heads * hd, generator=g) * 1.5).to(T16[dt])
    kb = None
    if masked:
        kb = torch.zeros(items, S)
        for i in range(items):
            n = int(torch.randint(1, S + 1, (1,), generator=g))
            kb[i, n:] = -1.0
        kb[0, :] = -1.0                       # an all-masked (padding) item attends uniformly
    return qkv, kb


def head_major(qkv, items, S, heads, hd=64):
    """row-major qkv as the 64-wide kernels read it, [item][head][q|k|v][S][hd], on the device"""
    return qkv.view(items, S, 3, heads, hd).permute(0, 3, 2, 1, 4).contiguous().cuda()


def run(lib, entry, dt, qkvd, kbd, items, S, heads, rows, hd=64):
    """One launch of `entry` into a buffer with a guard row behind it; the `rows` output rows, on the device."""
    out = torch.full((rows + 1, heads * hd), 7.0, dtype=T16[dt], device="cuda")
    _lib.check(getattr(lib, entry)(dt, qkvd.data_ptr(), kbd.data_ptr() if kbd is not None else None, out.data_ptr(), items, S, heads,
                                   stream()), entry)
    torch.cuda.synchronize()
    assert (out[rows] == 7.0).all(), f"{entry}: wrote behind its output"
    return out[:rows]
