"""GPU tests of the frozen DeBERTa-v2/v3 text tower: the disentangled attention kernel and its CLS form as primitives against float64, the
table projection, the towers of the HuggingFace golden (tests/golden/deberta_v2.npz) through every entry point, and the model on top
(`ModelMM` with the `b30` text tower: a training step, `evaluate.build_tap_cache`, the item-store route).
Host side: tests/test_deberta_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import deberta_oracle as DO  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import _lib, encoders, evaluate, itemstore, synth, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

F16, BF16 = _lib.IISAN_F16, _lib.IISAN_BF16
T16 = {F16: torch.float16, BF16: torch.bfloat16}
PRIM_TOL = {F16: 2e-3, BF16: 1.6e-2}        # tests/test_gpu_primitives.py: relative to the output scale, one 16-bit rounding of the result
TAP_TOL = {F16: 1.5e-3, BF16: 1.2e-2}       # tests/test_gpu_encoders.py: test_full_size_taps_match_reference_golden
EBADSHAPE = -1


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- a. the attention primitive ---------------------------------------------------------------------------------------------------------

# (items, S, heads, span, masked).  S: one token, one tile minus / exactly / plus one, the reference's 30, every tile-count rung (32 | 64 | 128) and
# its neighbours; span 32 with S = span reaches table rows 1 .. 63; 130 items: more workgroups than CUs at 12 heads; (1, 30, 3): an odd
# number of (item, head) pairs, the idle half of the last workgroup of the two-pair kernel
ATTN_CASES = [(3, 1, 2, 256, False), (3, 2, 12, 256, True), (1, 15, 2, 256, True), (3, 16, 2, 256, False), (3, 17, 12, 256, True),
              (130, 30, 12, 256, True), (130, 30, 2, 256, False), (1, 30, 3, 256, True), (3, 33, 2, 256, True), (3, 64, 2, 256, False),
              (1, 127, 2, 256, True), (3, 128, 12, 256, True), (3, 128, 2, 256, False), (3, 17, 2, 32, True), (3, 32, 12, 32, False),
              # more workgroups than the 256 CUs hold on the 64- and the 128-word instantiations too: 840 and 540 (the 128-word image takes
              # 118 KiB of LDS: one workgroup per CU)
              (70, 64, 12, 256, True), (45, 128, 12, 256, True),
              # spans shorter than the padded title (S <= span < SP = 16 ceil(S / 16)): both ends of the table image in LDS are clamped
              # re-reads, and S == span reaches table row 2 span - 1
              (3, 5, 2, 5, True), (3, 17, 2, 17, False), (2, 100, 2, 100, True)]


@functools.lru_cache(maxsize=None)
def _attn_problem(items, S, heads, span, masked, dt):
    """16-bit-rounded operands (head-major qkv, the table image [H, 3, 2 span, 64]), the key bias, and the float64 references: the kernel's
    arithmetic, the same without the positional terms, the same with the tables indexed at j - i + span."""
    g = torch.Generator().manual_seed(S * 13 + heads + span)
    qkv = (torch.randn(items, heads, 3, S, 64, generator=g) * 1.5).to(T16[dt])
    rel = (torch.randn(heads, 3, 2 * span, 64, generator=g) * 1.5).to(T16[dt])
    kb = None
    if masked:
        kb = torch.zeros(items, S)
        for i in range(items):
            n = int(torch.randint(1, S + 1, (1,), generator=g))
            kb[i, n:] = -1.0
        kb[0, :] = -1.0                       # an all-masked (padding) item attends uniformly
    q, k, v = (qkv[:, :, i].double() for i in range(3))
    pq, pk = rel[:, 0].double(), rel[:, 1].double()
    ctx = lambda **kw: DO.disentangled_attention(q, k, v, pq, pk, kb, span, **kw).transpose(1, 2).reshape(items, S, heads * 64)
    return qkv, rel, kb, ctx(), ctx(c2p=False, p2c=False), ctx(flip=True)


def _run_attn(lib, dt, qkv, rel, kb, items, S, heads, span, cls=False):
    qd, rd = qkv.cuda(), rel.cuda()
    kbd = kb.cuda() if kb is not None else None
    out = torch.full((items, heads * 64) if cls else (items * S, heads * 64), float("nan"), dtype=T16[dt], device="cuda")
    fn = lib.iisan_attention_cls16_disent if cls else lib.iisan_attention16_disent
    _lib.check(fn(dt, qd.data_ptr(), rd.data_ptr(), kbd.data_ptr() if kbd is not None else None, out.data_ptr(), items, S, heads, span, _stream()),
               "attention16_disent")
    torch.cuda.synchronize()
    return out.cpu().double()


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("case", ATTN_CASES)
def test_disentangled_attention_vs_float64(lib, dt, case):
    """iisan_attention16_disent against float64 on the 16-bit-rounded operands at the bound of test_attention16_vs_torch: the same two
    roundings remain (P and O), the three score terms accumulate in fp32.  Then the CLS form against float64 and against row 0 of the full
    kernel at the same bound."""
    items, S, heads, span, masked = case
    qkv, rel, kb, ref, _, _ = _attn_problem(*case, dt)
    got = _run_attn(lib, dt, qkv, rel, kb, items, S, heads, span).view(items, S, -1)
    tol = 2.5 * PRIM_TOL[dt] * ref.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"disent dt={dt} {case}: max err {err:.3e}, bound {tol:.3e}")
    assert torch.isfinite(got).all() and err <= tol, f"disent dt={dt} {case}: max err {err:.3e} > {tol:.3e}"
    cls = _run_attn(lib, dt, qkv, rel, kb, items, S, heads, span, cls=True)
    e64, efull = (cls - ref[:, 0]).abs().max().item(), (cls - got[:, 0]).abs().max().item()
    print(f"  cls form: vs float64 {e64:.3e}, vs row 0 of the full kernel {efull:.3e}")
    assert e64 <= tol and efull <= tol, f"cls dt={dt} {case}: {e64:.3e} / {efull:.3e} > {tol:.3e}"


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("case", [(3, 30, 12, 256, True), (3, 128, 2, 256, False), (3, 32, 2, 32, True)])
def test_disentangled_attention_negative_controls(lib, dt, case):
    """The check above must tell the kernel's arithmetic from its two nearest wrong ones: no positional terms, and the tables indexed at
    j - i + span.  The separation is asserted first — a control that could not discriminate is itself a failure."""
    items, S, heads, span, masked = case
    qkv, rel, kb, ref, nopos, flip = _attn_problem(*case, dt)
    tol = 2.5 * PRIM_TOL[dt] * ref.abs().max().item()
    for what, wrong in (("no positional terms", nopos), ("delta' = j - i + span", flip)):
        sep = (wrong - ref).abs().max().item()
        assert sep > 4 * tol, f"{what}: the references differ by {sep:.3e} only, bound {tol:.3e}: the control cannot discriminate"
    got = _run_attn(lib, dt, qkv, rel, kb, items, S, heads, span).view(items, S, -1)
    assert (got - ref).abs().max().item() <= tol
    for what, wrong in (("no positional terms", nopos), ("delta' = j - i + span", flip)):
        err = (got - wrong).abs().max().item()
        print(f"{what}: kernel vs the wrong reference {err:.3e}, bound {tol:.3e}")
        assert err > tol, f"{what}: the check accepts the wrong arithmetic ({err:.3e} <= {tol:.3e})"
        # ... and the CLS row alone (the CLS form is checked against it)
        assert (got[:, 0] - wrong[:, 0]).abs().max().item() > tol, what


UNREACHABLE_CASES = [(3, 30, 12, 256, True), (3, 17, 2, 32, True), (2, 100, 2, 256, False)]
POISON_ROW = 30000.0        # finite in fp16 and bf16; a 64-term dot product with |q| < 8 stays finite in fp32 (64 * 8 * 30,000 = 1.5e7)


@functools.lru_cache(maxsize=None)
def _unreachable_problem(items, S, heads, span, masked, dt):
    """q, k, v (|.| < 8) and two table images that agree on the rows a real (query, key) pair of an S-word title reads, d = i - j + span in
    [span - S + 1, span + S - 1]: every other row is zero in the first and +-30,000 in alternating sign in the second."""
    g = torch.Generator().manual_seed(S * 17 + heads + span)
    qkv = (torch.randn(items, heads, 3, S, 64, generator=g) * 1.5).clamp_(-7.5, 7.5).to(T16[dt])
    rel = (torch.randn(heads, 3, 2 * span, 64, generator=g) * 1.5).to(T16[dt])
    d = torch.arange(2 * span)
    dead = (d < span - S + 1) | (d > span + S - 1)
    assert dead.sum() == 2 * span - (2 * S - 1) and not dead[span]
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0) * torch.where(d % 2 == 0, 1.0, -1.0)[:, None]
    zero, poison = rel.clone(), rel.clone()
    zero[:, :, dead] = 0
    poison[:, :, dead] = (sign[dead] * POISON_ROW).to(T16[dt])
    assert torch.isfinite(poison).all() and poison[:, :, dead].float().abs().min() > 29000
    kb = None
    if masked:
        kb = torch.zeros(items, S)
        for i in range(1, items):
            kb[i, int(torch.randint(1, S + 1, (1,), generator=g)):] = -1.0
        kb[0, :] = -1.0
    return qkv, zero, poison, kb


def _disent_ref(qkv, rel, kb, span):
    q, k, v = (qkv[:, :, i].double() for i in range(3))
    items, heads, S = q.shape[:3]
    return DO.disentangled_attention(q, k, v, rel[:, 0].double(), rel[:, 1].double(), kb, span).transpose(1, 2).reshape(items, S, heads * 64)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("case", UNREACHABLE_CASES)
def test_unreachable_table_rows_have_no_influence(lib, dt, case):
    """The kernel header's promise: table rows no real (query, key) pair can reach — the rows the LDS image holds for pad keys and pad
    queries, and every row the image never holds — have no influence.  The full kernel and the CLS form, run on a table whose unreachable
    rows are zero and on one where they hold +-30,000, give the same, finite bits."""
    items, S, heads, span, masked = case
    qkv, zero, poison, kb = _unreachable_problem(*case, dt)
    assert qkv.float().abs().max() < 8
    for cls in (False, True):
        a = _run_attn(lib, dt, qkv, zero, kb, items, S, heads, span, cls=cls)
        b = _run_attn(lib, dt, qkv, poison, kb, items, S, heads, span, cls=cls)
        what = f"{'cls form' if cls else 'full kernel'} dt={dt} {case}"
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), what
        assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} elements depend on rows no real pair reaches"


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("case", UNREACHABLE_CASES)
def test_control_a_reachable_table_row_has_influence(dt, case):
    """On the CPU, so that the row classification above cannot be vacuous: the float64 reference does not see the unreachable rows either,
    and with ONE reachable row changed (d = span, the diagonal i == j) it moves by more than the bound of the primitive test."""
    items, S, heads, span, masked = case
    qkv, zero, poison, kb = _unreachable_problem(*case, dt)
    ref = _disent_ref(qkv, zero, kb, span)
    assert torch.equal(_disent_ref(qkv, poison, kb, span), ref)
    tol = 2.5 * PRIM_TOL[dt] * ref.abs().max().item()
    moved = zero.clone()
    moved[:, :, span] = -moved[:, :, span]
    sep = (_disent_ref(qkv, moved, kb, span) - ref).abs().max().item()
    print(f"dt={dt} {case}: one reachable row changed moves the reference by {sep:.3e}, bound {tol:.3e}")
    assert sep > tol
    # ... on the CLS row too (the CLS form reads d = span - j: the row is reachable from query 0 through key 0)
    assert (_disent_ref(qkv, moved, kb, span)[:, 0] - ref[:, 0]).abs().max().item() > tol


@pytest.mark.parametrize("cls", [False, True])
@pytest.mark.parametrize("S,span,why", [(129, 256, "sequence length 129"), (17, 16, "sequence length 17"), (8, 257, "span 257"), (0, 16, "sequence length 0")])
def test_disentangled_attention_refusals(lib, cls, S, span, why):
    """S = 129, S > span, a span past 256: IISAN_EBADSHAPE, nothing launched (the output keeps its fill)."""
    buf = torch.zeros(1 << 16, dtype=torch.float16, device="cuda")
    out = torch.full((4096,), 7.0, dtype=torch.float16, device="cuda")
    fn = lib.iisan_attention_cls16_disent if cls else lib.iisan_attention16_disent
    rc = fn(F16, buf.data_ptr(), buf.data_ptr(), None, out.data_ptr(), 1, S, 2, span, _stream())
    torch.cuda.synchronize()
    assert rc == EBADSHAPE and why in lib.iisan_last_error().decode(), lib.iisan_last_error()
    assert (out == 7.0).all()


# ---- b. the table projection -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("span,D", [(16, 128), (256, 128), (16, 768), (256, 768), (100, 384), (1, 128), (256, 1024)])
def test_table_projection_vs_float64(lib, dt, span, D):
    """iisan_deberta_rel_project: [layers][heads][3][2 span][64], third 0 = query_proj(LN(table)), third 1 = key_proj(LN(table)), against
    float64 LayerNorm + Linear on the 16-bit-rounded matrices, relative to the output scale.  (100, 384): a table that ends inside a
    256-row tile; (1, 128): the smallest table, two rows; 384 and 1024: every width a DeBERTa tower has."""
    cfg = weights.DebertaConfig(hidden=D, layers=2, heads=D // 64, mlp=256, vocab=64, position_buckets=span)
    w = weights.make_deberta_weights(cfg, seed=71, std=0.05)
    pk = encoders.PackedDeberta(w, cfg, "cuda", dt)
    assert pk.struct.rel_proj and pk._rel.numel() == 2 * 3 * 2 * span * D * 2 == lib.iisan_deberta_rel_bytes(C.byref(pk.struct))
    got = pk._rel.view(T16[dt]).view(2, D // 64, 3, 2 * span, 64).cpu().double()
    w16 = {k: (v.to(T16[dt]) if k.endswith("qkv_w") else v) for k, v in w.items()}
    for l in range(2):
        pq, pkk = DO.rel_tables(w16, cfg, l)
        for third, ref in ((0, pq), (1, pkk)):
            err, scale = (got[l, :, third] - ref).abs().max().item(), ref.abs().max().item()
            print(f"span {span} D {D} dt={dt} layer {l} third {third}: max err {err:.3e}, bound {PRIM_TOL[dt] * scale:.3e}")
            assert err <= PRIM_TOL[dt] * scale
    # refusals: a workspace that is too small, a span outside 1 .. 256
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    assert lib.iisan_deberta_rel_project(C.byref(pk.struct), pk._rel.data_ptr(), ws.data_ptr(), ws.numel(), _stream()) != 0
    assert "workspace too small" in lib.iisan_last_error().decode()


# ---- c. the towers ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tower(name, dt=F16):
    cfg, w, x, gold = DO.load_golden(name)
    return cfg, w, x, gold, encoders.PackedBert(w, cfg, "cuda", dt)


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("name", sorted(DO.TOWERS))
def test_deberta_taps_match_the_huggingface_golden(name, dt):
    """Every CLS tap of the four golden towers against HF's own hidden states, per tap layer, at the project's tap bound; the all-masked
    slot's taps are finite and inside the same bound on their own.  Measured values: profiles/deberta_tower.md."""
    cfg, w, x, gold, pk = _tower(name, dt)
    assert type(pk) is encoders.PackedDeberta and pk.struct.rel_proj
    layers = list(range(cfg.layers + 1))
    got = pk.forward_taps(x.cuda(), layers).cpu()
    assert torch.isfinite(got).all()
    errs = DO.tap_errors(got, gold)
    print(f"{name} dt={dt} tap errors: " + " ".join(f"{e:.2e}" for e in errs))
    # tap 0 is LayerNorm(word row) * mask in fp32: no 16-bit arithmetic touches the CLS row before block 0
    assert errs[0] < 1e-5, errs[0]
    for l, e in enumerate(errs):
        assert e < TAP_TOL[dt], f"{name} tap {l}: {e:.3e}"
    # the padding item (slot 0: ids and mask zero): hidden state 0 is exactly zero, the deeper taps are those of HF
    assert (got[0, 0] == 0).all()
    pad = DO.tap_errors(got[:1, 1:], gold[:1, 1:])
    print(f"{name} dt={dt} all-masked slot: " + " ".join(f"{e:.2e}" for e in pad))
    assert max(pad) < TAP_TOL[dt], pad
    # a subset of the taps is the same rows
    assert torch.equal(pk.forward_taps(x.cuda(), [0, 1]).cpu()[:, 0], got[:, 0])


@pytest.mark.parametrize("name", sorted(DO.TOWERS))
def test_deberta_entry_points_chunks_tables_and_workspace_are_bit_equal(lib, name):
    """Plain, indexed and dropout-entry (drop = NULL, and both probabilities 0) calls; chunk_items 1 / 2 / 0; rel_proj given or projected
    by the call; a poisoned workspace: the same bits.  A non-zero probability is refused before any launch."""
    cfg, w, x, gold, pk = _tower(name)
    xs = x.cuda()
    layers = list(range(cfg.layers + 1))
    want = pk.forward_taps(xs, layers)
    index = torch.tensor([3, -1, 0, 2, 2, 4, 1], device="cuda")          # pads: negative and == rows: the all-masked item
    ti = pk.forward_taps_indexed(xs, index, layers)
    assert torch.equal(ti, torch.stack([want[i] if 0 <= i < 4 else want[0] for i in index.tolist()]))
    assert torch.equal(pk.forward_taps(xs, layers, dropout=(0.0, 0.0, 5)), want)
    assert torch.equal(pk.forward_taps_indexed(xs, index, layers, dropout=(0.0, 0.0, 5)), ti)
    nbytes = lib.iisan_bert_forward_taps_ws_bytes(C.byref(pk.struct), 4, x.shape[1] // 2, 0)
    got = pk._taps_call("iisan_bert_forward_taps_dropout", (xs.data_ptr(), 0, None, 4, x.shape[1] // 2), 4, layers, 0, nbytes, xs.device, extra=(None,))
    assert torch.equal(got, want)
    for chunk in (1, 2):
        assert torch.equal(pk.forward_taps(xs, layers, chunk_items=chunk), want)
        assert torch.equal(pk.forward_taps_indexed(xs, index, layers, chunk_items=chunk), ti)
    # the call projects the tables itself: a larger workspace for such a struct only, the same bits
    own = encoders.PackedDeberta(w, cfg, "cuda", F16, project_tables=False)
    assert not own.struct.rel_proj
    grown = lib.iisan_bert_forward_taps_ws_bytes(C.byref(own.struct), 4, x.shape[1] // 2, 0)
    assert grown >= nbytes + lib.iisan_deberta_rel_bytes(C.byref(own.struct)) + lib.iisan_deberta_rel_ws_bytes(C.byref(own.struct))
    assert torch.equal(own.forward_taps(xs, layers), want)
    assert torch.equal(own.forward_taps(xs, layers, chunk_items=1), want)
    # a poisoned workspace (NaN patterns in every word) changes nothing: no buffer is read before it is written
    for p in (pk, own):
        p.ws.buf.view(torch.int16).fill_(0x7E00)
        assert torch.equal(p.forward_taps(xs, layers), want)
        p.ws.buf.fill_(0xFF)
        assert torch.equal(p.forward_taps(xs, layers, chunk_items=2), want)
    # a too-small workspace and train-mode dropout are refused before any launch
    rc = lib.iisan_bert_forward_taps(C.byref(own.struct), xs.data_ptr(), 4, x.shape[1] // 2, (C.c_int32 * 1)(1), 1, want.data_ptr(), 0,
                                     own.ws.buf.data_ptr(), nbytes, _stream())
    assert rc != 0 and "workspace too small" in lib.iisan_last_error().decode()
    drop = _lib.BertDropout(0.1, 0.0, 1)
    rc = lib.iisan_bert_forward_taps_dropout(C.byref(pk.struct), xs.data_ptr(), 0, None, 4, x.shape[1] // 2, (C.c_int32 * 1)(1), 1, want.data_ptr(), 0,
                                             C.byref(drop), pk.ws.buf.data_ptr(), pk.ws.buf.numel(), _stream())
    assert rc == EBADSHAPE and "eval mode only" in lib.iisan_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(pk.forward_taps(xs, layers), want)


@pytest.mark.parametrize("name", sorted(DO.TOWERS))
def test_deberta_full_blocks_and_resid32_routes(name):
    """full_blocks = 1 (every block on every token): the shallower taps are bit-equal to the default and the last one, which the CLS-only
    block (the CLS form of the attention) produces by default, is within the tap bound of the golden; the difference between the two routes
    is printed.  The fp32 residual stream of the dev switch resid32 = 1 is within the tap bound too."""
    cfg, w, x, gold, pk = _tower(name)
    xs = x.cuda()
    layers = list(range(cfg.layers + 1))
    want = pk.forward_taps(xs, layers)
    pk.full_blocks = True
    try:
        full = pk.forward_taps(xs, layers)
    finally:
        pk.full_blocks = False
    assert torch.equal(full[:, :-1], want[:, :-1])
    e_full = DO.tap_errors(full.cpu(), gold)[-1]
    diff = DO.tap_errors(want[:, -1:].cpu(), full[:, -1:].cpu())[0]
    print(f"{name}: last tap, all-token route vs golden {e_full:.2e}; CLS-only route vs all-token route {diff:.2e}")
    assert e_full < TAP_TOL[F16]
    with _lib.dev(resid32=1):
        r32 = pk.forward_taps(xs, layers)
    e32 = DO.tap_errors(r32.cpu(), gold)
    print(f"{name}: resid32 tap errors " + " ".join(f"{e:.2e}" for e in e32))
    assert e32[0] < 1e-5 and max(e32) < TAP_TOL[F16], e32


@pytest.mark.parametrize("name", ["n8", "b30"])
def test_taps_do_not_depend_on_the_ids_at_padded_positions(name):
    """Every tap is bit-independent of the ids stored at padded positions: the embedding step multiplies a masked token's row by its mask
    bit, so the tower never sees which word sat there (the float64 statement of the same: tests/test_deberta_host.py)."""
    cfg, w, x, gold, pk = _tower(name)
    W = x.shape[1] // 2
    y = x.clone()
    pad = y[:, W:] == 0
    y[:, :W][pad] = torch.randint(1, cfg.vocab, (int(pad.sum()),), generator=torch.Generator().manual_seed(5))
    assert not torch.equal(x, y)
    layers = list(range(cfg.layers + 1))
    assert torch.equal(pk.forward_taps(x.cuda(), layers), pk.forward_taps(y.cuda(), layers))


def test_deberta_forward_refusals_before_any_launch(lib):
    """words > span / 2, words > 128, a span outside 1 .. 256, a hidden size outside the executor's set: IISAN_EBADSHAPE, the taps untouched."""
    cfg, w, x, gold, pk = _tower("n8")
    taps = torch.full((4, 1, cfg.hidden), 7.0, device="cuda")
    ws = torch.empty(1 << 26, dtype=torch.uint8, device="cuda")
    def call(struct, words):
        text = torch.zeros(4, 2 * words, dtype=torch.int64, device="cuda")
        rc = lib.iisan_bert_forward_taps(C.byref(struct), text.data_ptr(), 4, words, (C.c_int32 * 1)(1), 1, taps.data_ptr(), 0, ws.data_ptr(), ws.numel(), _stream())
        torch.cuda.synchronize()
        return rc, lib.iisan_last_error().decode()
    rc, msg = call(pk.struct, 9)
    assert rc == EBADSHAPE and "span / 2" in msg, msg
    big = _tower("b30")[4]
    rc, msg = call(big.struct, 129)
    assert rc == EBADSHAPE and ("span / 2" in msg or "128" in msg), msg
    s = type(pk.struct).from_buffer_copy(pk.struct)
    s.span = 257
    rc, msg = call(s, 8)
    assert rc == EBADSHAPE and "span" in msg, msg
    s.span, s.hidden = 16, 512
    rc, msg = call(s, 8)
    assert rc == EBADSHAPE and "512" in msg, msg
    assert (taps == 7.0).all()


def test_a_bert_tower_keeps_its_bits_around_a_deberta_call():
    """A BERT struct (the new fields zero) in the same process: one call before and one after a DeBERTa call give the same bits, and those
    bits are the golden route's (tests/golden/encoders_full.npz is held by tests/test_gpu_encoders.py; here: the float64 oracle's bound)."""
    from oracle import iisan_oracle as O
    bcfg = weights.BertConfig(hidden=768, layers=2, heads=12, mlp=512, vocab=512, max_pos=64)
    bw = weights.make_bert_weights(bcfg, seed=12)
    bert = encoders.PackedBert(bw, bcfg, "cuda")
    assert type(bert) is encoders.PackedBert and not bert.struct.rel_emb and bert.struct.span == 0
    text = DO.texts(30, 77).cuda()
    before = bert.forward_taps(text, [0, 1, 2])
    cfg, w, x, gold, pk = _tower("b30")
    pk.forward_taps(x.cuda(), [0, 1, 2])
    after = bert.forward_taps(text, [0, 1, 2])
    assert torch.equal(before, after)
    ref = O.bert_cls_taps(text.cpu(), bw, bcfg)
    assert max(DO.tap_errors(after.cpu(), ref)) < TAP_TOL[F16]


# ---- d. the model on top ----------------------------------------------------------------------------------------------------------------

E2E_VIT = weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=32, patch=16)
WORDS, ITEM_NUM = 30, 40


def _model(train=True):
    """`ModelMM` Uncached on a ViT toy and the `b30` DeBERTa tower (768 / 12 / 2 layers, 30-word titles), no dropout anywhere."""
    from iisan_amd.model import encoders as menc
    dcfg, dw = DO.TOWERS["b30"][0], weights.make_deberta_weights(DO.TOWERS["b30"][0], seed=DO.TOWERS["b30"][2])
    vw = weights.make_vit_weights(E2E_VIT, seed=11)
    args = helpers.make_args(side_adapter_vit_list="0,1", side_adapter_bert_list="0,1", num_words_title=WORDS, drop_rate=0.0,
                             adapter_dropout_rate=0.0, bert_model_load="deberta-v3-base")
    model = helpers.build_model(args, ITEM_NUM, synth.make_pop_prob(ITEM_NUM), vw, E2E_VIT, dw, dcfg, cached=False)
    assert type(model.mm_encoder.bert_encoder.text_encoders["title"].bert_model) is menc.FrozenDeberta
    P = weights.make_trainable_params(seed=101, n_side=3)
    helpers.load_trainables(model, P)
    model.train(train)
    return model, vw, dw, dcfg, P


def test_uncached_model_with_a_deberta_tower_matches_the_float64_oracle():
    """One training step of `ModelMM` on the DeBERTa text tower — `train_dropout` switched on, which a DeBERTa tower ignores: loss and the
    three item embeddings against `O.model_loss_from_taps` fed the float64 DeBERTa taps (and the oracle's ViT taps) at the 1e-3 relative of
    the e2e tests (fp16 encoder operands); gradients finite, every trainable tensor receives one."""
    b = synth.scientific_batch(bs=3, seed=31, lengths=[3, 11, 6], dup_items=True, res=32, words=WORDS, vocab=DO.VOCAB, item_num=ITEM_NUM)
    model, vw, dw, dcfg, P = _model()
    title = model.mm_encoder.bert_encoder.text_encoders["title"]
    title.train_dropout = True
    assert title.step_dropout() is None
    ids, lm, img, txt = b.ids.cuda().view(-1), b.log_mask.cuda(), b.images.cuda(), b.text.cuda()
    cv, (text, mm) = model.mm_encoder(img, txt)
    loss = model(ids, img, txt, lm, 0)
    loss.backward()
    with torch.no_grad():
        tc = O.vit_cls_taps(b.images, vw, E2E_VIT)
        tt = DO.deberta_cls_taps(b.text, dw, dcfg).float()
        ref, aux = O.model_loss_from_taps(b.ids, tc, tt, b.log_mask, b.pop_prob, P, O.side_layer_list("0,1", False))
    real = (b.ids.view(-1) != 0)
    for got, key in ((cv, "cv"), (text, "text"), (mm, "mm")):
        rel = ((got.detach().cpu().double() - aux[key].double())[real].norm() / aux[key].double()[real].norm()).item()
        print(f"{key}: rel {rel:.3e}")
        assert rel < 1e-3, f"{key}: rel {rel:.3e}"
    rel = abs(loss.item() - ref.item()) / abs(ref.item())
    print(f"loss {loss.item():.6f} oracle {ref.item():.6f} rel {rel:.2e}")
    assert rel < 1e-3
    taps = model.mm_encoder.bert_encoder.forward_taps(txt, [0, 1, 2]).cpu()
    assert max(DO.tap_errors(taps, tt)) < TAP_TOL[F16]
    n = 0
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), name
            n += 1
    assert n > 50


def test_tap_cache_and_item_store_routes_reproduce_the_direct_taps_bitwise():
    """`evaluate.build_tap_cache` (batches of 10 over 41 titles) and the `ItemStore` indexed route give the bits of one direct
    `forward_taps` call; the model's loss over the store equals the materialised batch's."""
    model, vw, dw, dcfg, P = _model()
    N = ITEM_NUM + 1            # a store holds a row for every item id of the model, row 0 the padding item
    images = synth.make_images(np.arange(N), 32, seed=5)
    text = torch.from_numpy(synth.make_text(np.arange(N), WORDS, DO.VOCAB, np.random.RandomState(0)))
    direct = model.mm_encoder.bert_encoder.forward_taps(text.cuda(), [0, 1, 2])
    taps_cv, taps_tx = evaluate.build_tap_cache(model, images.cuda(), text.cuda(), batch=10)
    assert taps_tx.shape == (N, 3, 768) and torch.equal(taps_tx, direct)
    assert max(DO.tap_errors(taps_tx.cpu(), DO.deberta_cls_taps(text, dw, dcfg))) < TAP_TOL[F16]
    cat = ((images * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)
    store = itemstore.ItemStore(cat.numpy(), text, "cuda")
    st_cv, st_tx = evaluate.build_tap_cache_from_store(model, store, batch=7)
    assert torch.equal(st_tx, direct)
    index = torch.tensor([5, 0, -1, 23, 5, N], device="cuda")
    got = model.mm_encoder.bert_encoder.forward_taps_indexed(store.text, index, [0, 1, 2])
    assert torch.equal(got, torch.stack([direct[i] if 0 < i < N else direct[0] for i in index.tolist()]))
