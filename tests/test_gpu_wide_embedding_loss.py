"""The in-batch loss (`iisan_inbatch_ce_fwd/bwd`, csrc/ce.hip) at `embedding_dim` 128, 192 and 256: the f32 passes over NE = E / 64
feature blocks, on the fused, row-pass and generic routes (the split-operand route is 64 wide: `ce_fast` 3 takes the fused passes).

The problems are those of `tests/test_gpu_ce_regimes.py` (`_problem` there: the seeds crc32("regime/bs/S"), the regimes, their structural
assertions and negative controls) with the width as a parameter instead of that module's constant 64 - restated here, because that
module's generator reads its own `E`.  Reference `O.inbatch_ce` in float64 on the same float32 inputs; bounds that file's own (loss 2e-5
relative, gradients 2e-4 of their scale + 1e-9), and its conditioning guard: the float32 oracle stays within 1/8 of each bound.  One
more wrong answer per problem: the float64 result on the first 64 features alone - a kernel that walks one feature block must not pass.
Measured errors: `profiles/wide_embedding.md`."""
import ctypes as C
import functools
import random
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from iisan_amd import _lib, ops, synth  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402
from test_gpu_abi_contracts import Guarded, _guards_intact  # noqa: E402
from test_gpu_ce_regimes import ALIGN, MASKV, _check, _errors, _fails, _left_padding, _oracle  # noqa: E402

IISAN_EBADSHAPE, IISAN_EWORKSPACE = -1, -2
WIDTHS = (128, 192, 256)
REGIMES = ("trained", "sharp", "ramp", "repeats5", "holes")
TRAINED_FAMILY = ("trained", "repeats5", "holes")
# seed offset per (regime, bs, S, E), as `RESEED` of test_gpu_ce_regimes.py: 0 unless that problem's structure is not the regime's
# (ramp at 4 x 16, E = 192, offset 0: the largest logit of 17 of 36 valid rows is late, the regime wants half)
RESEED = {("ramp", 4, 16, 192): 1}
ROW_SHAPES = [(7, 5), (37, 10), (6, 15)]
GENERIC_SHAPES = [(9, 3), (4, 16)]
# route name -> (dev switches, iisan_inbatch_ce_route_e's answer on a row-fixed shape)
ROUTES = {"default": ({}, 2), "fused": (dict(ce_fast=4), 2), "rowpass": (dict(ce_fast=2), 1), "generic": (dict(ce_fast=0), 0)}
CASES = [(bs, S, r) for bs, S in ROW_SHAPES for r in ROUTES] + [(bs, S, "default") for bs, S in GENERIC_SHAPES]


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _problem(regime, bs, S, E):
    """`test_gpu_ce_regimes.py::_problem` at width E: float32 inputs, the float64 loss and gradients, the conditioning guard, the
    structural assertions and the wrong answers of the negative controls.  Computed once per problem, shared by the routes."""
    seed = zlib.crc32(f"{regime}/{bs}/{S}".encode()) % (1 << 30) + RESEED.get((regime, bs, S, E), 0)
    rnd = random.Random(seed)
    lengths = [rnd.randint(2, S + 1) for _ in range(bs)]
    if regime == "repeats5":
        lengths[0] = S + 1
    n = max(40, bs * 3, 2 * (S + 1))
    rs = np.random.RandomState(seed)
    ids, log_mask = synth.make_ids(bs, S, n, rs, lengths)
    if regime == "repeats5":
        cat = min(5, S)
        real = ids != 0
        ids[real] = rs.randint(1, cat + 1, size=int(real.sum()))
        ids[0, S + 1 - cat:] = 1 + rs.permutation(cat)
    ids, log_mask = torch.from_numpy(ids), torch.from_numpy(log_mask)
    pop = synth.make_pop_prob(n)
    g = torch.Generator().manual_seed(seed)
    T, M = bs * S, bs * (S + 1)
    label = (torch.arange(bs)[:, None] * (S + 1) + torch.arange(1, S + 1)[None, :]).view(-1)
    if regime == "holes":
        on = torch.rand(bs, S, generator=g) < 0.6
        vals = torch.tensor([1.0, 2.5, -1.0])[torch.randint(0, 3, (bs, S), generator=g)]
        log_mask = torch.where(on, vals, torch.zeros(()))
        log_mask[:, -1] = vals[:, -1]

    align = None
    if regime in TRAINED_FAMILY:
        emb = torch.randn(n + 1, E, generator=g)
        score = emb[ids.view(-1)]
        unit = score[label] / score[label].norm(dim=1, keepdim=True)
        noise = 0.3 * torch.randn(T, E, generator=g)
        for align in ALIGN:
            prec = align * unit + noise
            with torch.no_grad():
                l64 = O.inbatch_ce(ids, score.double(), prec.double(), log_mask.double(), pop.double()).item()
            if l64 >= 0.1:
                break
    elif regime == "sharp":
        score, prec = 2 * torch.randn(M, E, generator=g), torch.randn(T, E, generator=g)
    elif regime == "ramp":
        score = torch.randn(M, E, generator=g) * (0.25 + 1.75 * torch.arange(M) / (M - 1))[:, None]
        prec = torch.randn(T, E, generator=g)
    else:
        raise KeyError(regime)

    loss, ds, dp = _oracle(ids, score, prec, log_mask, pop, torch.float64)
    with torch.no_grad():
        z, lab = O.inbatch_logits(ids, score.double(), prec.double(), log_mask.double(), pop.double())
    assert torch.equal(lab, label)
    valid = log_mask.reshape(-1) != 0
    live = z != MASKV
    p = dict(regime=regime, bs=bs, S=S, E=E, ids=ids, log_mask=log_mask, pop=pop, score=score, prec=prec, loss=loss, d_score=ds, d_prec=dp,
             align=align, max_logit=z[live].abs().max().item())

    # ---- the regime is what it says
    col_pad = torch.cat([log_mask, torch.ones(bs, 1)], 1).view(-1) == 0
    neg = live.clone()
    neg[torch.arange(T), label] = False
    no_negative = valid & ~neg.any(1)
    if regime == "repeats5":
        seq = ids.view(bs, S + 1)
        twice = (seq[:, None, 1:] == seq[:, :, None]).sum(1) >= 2
        assert bool(no_negative.any()), "no valid row is left without a negative"
        fired = (z == MASKV) & ~col_pad[None, :]
        p["masked"] = fired[valid].double().mean().item() / (~col_pad).double().mean().item()
        assert p["masked"] >= 0.5, p["masked"]
        assert bool((twice.reshape(-1) & valid).any()), "no valid row's label id occurs twice in its sequence"
    if regime == "ramp":
        late = z.masked_fill(~live, -float("inf")).argmax(1) >= M - max(16, M // 4)
        assert int((late & valid).sum()) * 2 >= int(valid.sum()), (int((late & valid).sum()), int(valid.sum()))
    if regime == "sharp":
        assert p["max_logit"] >= 50, p["max_logit"]
    if regime == "holes":
        assert bool((col_pad[label] & valid).any()), "no valid row's label column is padding"
        assert bool(((log_mask != 0) & (log_mask != 1)).any()) and not torch.equal(log_mask != 0, _left_padding(ids) != 0)
    if regime == "trained":
        assert 0.1 <= loss <= 3.0, loss
    assert loss >= 0.1, loss

    # ---- the reference is well conditioned: float32 arithmetic alone stays within 1/8 of every bound
    l32, ds32, dp32 = _oracle(ids, score, prec, log_mask, pop, torch.float32)
    p["floor"] = _errors(l32, ds32, dp32, p)
    try:
        _check(l32, ds32, dp32, p, frac=0.125)
    except AssertionError as e:
        raise AssertionError(f"an ill-conditioned reference ({regime}, {bs}, {S}, E = {E}): the float32 oracle misses 1/8 of the bounds: {e}") from None

    # ---- wrong answers the check has to reject
    wrong = {"loss x (1 + 1e-4)": (loss * (1 + 1e-4), ds, dp)}
    zeroed = ds.clone()
    zeroed[int(ds.abs().max(1).values.argmax())] = 0
    wrong["largest d_score row zeroed"] = (loss, zeroed, dp)
    if E > 64:                                   # (64 itself serves the route-agreement test alone)
        l1, ds1, dp1 = _oracle(ids, score[:, :64].contiguous(), prec[:, :64].contiguous(), log_mask, pop, torch.float64)
        wrong["the first 64 features only"] = (l1, torch.cat([ds1, torch.zeros(M, E - 64, dtype=ds1.dtype)], 1),
                                               torch.cat([dp1, torch.zeros(T, E - 64, dtype=dp1.dtype)], 1))
    if regime == "repeats5":
        wrong["no false-negative mask"] = _oracle(torch.arange(M).view(bs, S + 1), score, prec, log_mask, pop[ids.view(-1)], torch.float64)
    if regime == "holes":
        wrong["left-padding log_mask"] = _oracle(ids, score, prec, _left_padding(ids), pop, torch.float64)
    p["wrong"] = wrong
    return p


def _gpu(lib, p, knobs, want):
    """One forward + backward of `ops.InbatchCeFn` on the switches; the route and the ce16 counter asserted while they are set."""
    bs, S, E = p["bs"], p["S"], p["E"]
    if S < 5 or S >= 16:
        want = 0
    sd, pd = p["score"].cuda().requires_grad_(True), p["prec"].cuda().requires_grad_(True)
    ids, lm, pop = p["ids"].view(-1).cuda(), p["log_mask"].cuda(), p["pop"].cuda()
    with _lib.dev(**knobs):
        got = lib.iisan_inbatch_ce_route_e(bs, S, E)
        assert got == want, (knobs, got, want)
        before = _lib.dev_get("count:ce16")
        loss = ops.InbatchCeFn.apply(ids, sd, pd, lm, pop)
        loss.backward()
        torch.cuda.synchronize()
        assert _lib.dev_get("count:ce16") == before, "the split-operand route ran at a wide width"
    return loss.detach().cpu(), sd.grad.cpu(), pd.grad.cpu(), want


@pytest.mark.parametrize("bs,S,route", CASES, ids=[f"{bs}x{S}-{r}" for bs, S, r in CASES])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("E", WIDTHS)
def test_wide_inbatch_ce_matches_the_fp64_oracle_on_every_route(lib, E, regime, bs, S, route):
    """`InbatchCeFn` at E = 128 / 192 / 256 against `O.inbatch_ce` in float64: loss within 2e-5 relative, d_score and d_prec within 2e-4
    of their scale + 1e-9.  Shapes as in test_gpu_ce_regimes.py: (7, 5) three Y tiles, one wave without any; (37, 10) RS1 = 11, a
    partial last tile; (6, 15) RS1 = 16; (9, 3) and (4, 16) the generic kernel on default switches."""
    p = _problem(regime, bs, S, E)
    _check(p["loss"], p["d_score"], p["d_prec"], p)
    for what, (l, ds, dp) in p["wrong"].items():
        assert _fails(_check, l, ds, dp, p), f"the bounds accept '{what}': the case does not test what it claims"
    knobs, want = ROUTES[route]
    loss, ds, dp, want = _gpu(lib, p, knobs, want)
    el, es, ep = _errors(loss.item(), ds, dp, p)
    print(f"wide-ce E={E} {regime} bs={bs} S={S} route={route}({want}): loss {p['loss']:.4g} err {el:.2e}, d_score {es:.2e}, d_prec {ep:.2e}, "
          f"max|logit| {p['max_logit']:.1f}; float32 oracle {p['floor'][0]:.1e} / {p['floor'][1]:.1e} / {p['floor'][2]:.1e}")
    _check(loss.item(), ds, dp, p)


@pytest.mark.parametrize("E", WIDTHS)
def test_the_split_operand_switch_takes_the_fused_f32_passes_at_a_wide_width(lib, E):
    """`ce_fast` 3 (the split-operand route at every size) at E > 64: `iisan_inbatch_ce_route_e` answers 2, `count:ce16` does not move
    (asserted in `_gpu`), and the result holds the bounds."""
    p = _problem("trained", 37, 10, E)
    loss, ds, dp, _ = _gpu(lib, p, dict(ce_fast=3), 2)
    _check(loss.item(), ds, dp, p)


def _three_routes(lib, E):
    """{regime: (problem, {route: (loss, d_score, d_prec)})} on (37, 10), every regime"""
    out = {}
    for regime in REGIMES:
        p = _problem(regime, 37, 10, E)
        out[regime] = (p, {r: _gpu(lib, p, *ROUTES[r])[:3] for r in ("fused", "rowpass", "generic")})
    return out


@pytest.mark.parametrize("E", WIDTHS)
def test_the_three_routes_agree_at_a_wide_width_as_they_agree_at_64(lib, E):
    """Loss, d_score and d_prec of the fused, row-pass and generic routes on (37, 10).  What holds at 64 is established here by running
    the three at 64: a pair of routes agrees to the bit on a gradient tensor when it does so at 64 on EVERY regime, and on the loss
    when at 64 the loss AND d_score are equal to the bit on every regime.  (The loss alone does not tell: it is one rounded scalar, the
    mean of 370 rows.  At 64 the fused and the row-pass loss are the same float on all five regimes, yet their d_score - the same
    column pass fed with each forward's lse - differs, so the row sums are not the same numbers; at 128 and 192 two of the ten losses
    are one ulp apart.)  Every such pair has to be equal to the bit at E, on `trained` and on the other regimes (the pieces state every
    floating-point order once, at every width).  A pair that differs at 64 (another exp, the fused pass's rescaling) may differ at E by
    what two results inside the bounds of the oracle test can: twice those bounds, of the float64 result's scale."""
    at64, wide = _three_routes(lib, 64), _three_routes(lib, E)
    names = ("loss", "d_score", "d_prec")
    for a, b in (("fused", "rowpass"), ("fused", "generic"), ("rowpass", "generic")):
        for i, what in enumerate(names):
            same64 = all(torch.equal(r[a][i], r[b][i]) and (i > 0 or torch.equal(r[a][1], r[b][1])) for _, r in at64.values())
            for regime, (p, r) in wide.items():
                scale = (abs(p["loss"]), p["d_score"].abs().max().item(), p["d_prec"].abs().max().item())[i]
                same = torch.equal(r[a][i], r[b][i])
                diff = (r[a][i].double() - r[b][i].double()).abs().max().item()
                print(f"wide-ce agreement E={E} {regime} {a} vs {b} {what}: bit-equal at 64 on every regime {same64}, at {E} {same} "
                      f"(max diff {diff:.2e}, scale {scale:.2e})")
                if same64:
                    assert same, f"{a} and {b} agree to the bit on {what} at 64 and differ at {E} ({regime}) by {diff:.3e}"
                else:
                    assert diff <= 2 * ((2e-5 if i == 0 else 2e-4) * scale + (0 if i == 0 else 1e-9)), (regime, a, b, what, diff)


class _Call:
    """One raw loss call at width `E` (operands of width `Eop`) with workspace, loss and gradients between guard zones."""

    def __init__(self, lib, bs, S, E, ws_bytes=None):
        p = _problem("trained", bs, S, E)
        self.lib, self.bs, self.S, self.E, self.p = lib, bs, S, E, p
        self.ids, self.lm, self.pop = p["ids"].view(-1).cuda(), p["log_mask"].cuda(), p["pop"].cuda()
        self.score, self.prec = p["score"].cuda(), p["prec"].cuda()
        self.need = lib.iisan_inbatch_ce_ws_bytes_e(bs, S, E) if ws_bytes is None else ws_bytes
        self.ws = Guarded(self.need, torch.uint8)
        self.loss = Guarded(4, init=torch.tensor([float("nan")]))
        self.d_score = Guarded.like(p["score"], init=torch.full_like(p["score"], float("nan")))
        self.d_prec = Guarded.like(p["prec"], init=torch.full_like(p["prec"], float("nan")))
        self.tok = C.c_uint64(0)

    def fwd(self, Ein=None, ws_bytes=None):
        return self.lib.iisan_inbatch_ce_fwd(self.ids.data_ptr(), self.score.data_ptr(), self.prec.data_ptr(), self.lm.data_ptr(),
                                             self.pop.data_ptr(), self.pop.numel(), self.bs, self.S, self.E if Ein is None else Ein,
                                             self.loss.ptr, self.ws.ptr, self.need if ws_bytes is None else ws_bytes, C.byref(self.tok),
                                             _stream())

    def bwd(self, Ein=None, token=None, ws_bytes=None):
        return self.lib.iisan_inbatch_ce_bwd(self.ids.data_ptr(), self.score.data_ptr(), self.prec.data_ptr(), self.lm.data_ptr(),
                                             self.pop.data_ptr(), self.bs, self.S, self.E if Ein is None else Ein, 1.0, self.d_score.ptr,
                                             self.d_prec.ptr, self.ws.ptr, self.need if ws_bytes is None else ws_bytes,
                                             self.tok.value if token is None else token, _stream())

    def guards(self):
        return dict(ws=self.ws, loss=self.loss, d_score=self.d_score, d_prec=self.d_prec)

    def bits(self):
        torch.cuda.synchronize()
        return {k: v.bits() for k, v in self.guards().items()}

    def unchanged(self, before):
        now = self.bits()
        return all(torch.equal(now[k], before[k]) for k in before)


def test_widths_outside_the_set_and_foreign_tokens_are_refused_before_any_launch(lib):
    """`Ein` 32 / 96 / 320: IISAN_EBADSHAPE from the forward and the backward, the width in the message, -1 / 0 from the two queries; a
    forward token of width 128 handed to a backward call with `Ein` = 64 and the reverse: IISAN_EBADSHAPE; a workspace one byte short
    of `iisan_inbatch_ce_ws_bytes_e`: IISAN_EWORKSPACE.  Every time the workspace, the loss and both gradients keep their prefill."""
    bs, S = 37, 10
    big = lib.iisan_inbatch_ce_ws_bytes(bs, S)
    assert big >= lib.iisan_inbatch_ce_ws_bytes_e(bs, S, 256)        # (the 64-wide workspace holds the split route's images)
    c = _Call(lib, bs, S, 128, ws_bytes=big)
    before = c.bits()
    for bad in (32, 96, 320):
        assert lib.iisan_inbatch_ce_route_e(bs, S, bad) == -1 and lib.iisan_inbatch_ce_ws_bytes_e(bs, S, bad) == 0
        assert c.fwd(Ein=bad) == IISAN_EBADSHAPE
        assert b"embedding_dim" in lib.iisan_last_error() and str(bad).encode() in lib.iisan_last_error()
        assert c.tok.value == 0
    assert c.unchanged(before)
    _lib.check(c.fwd(), "iisan_inbatch_ce_fwd")
    tok128 = c.tok.value
    assert (tok128 >> 48) & 0xFF == 1
    before = c.bits()
    for bad in (32, 96, 320):
        assert c.bwd(Ein=bad) == IISAN_EBADSHAPE
        assert b"embedding_dim" in lib.iisan_last_error() and str(bad).encode() in lib.iisan_last_error()
    assert c.bwd(Ein=64) == IISAN_EBADSHAPE and b"fwd_token" in lib.iisan_last_error()
    assert c.bwd(ws_bytes=lib.iisan_inbatch_ce_ws_bytes_e(bs, S, 128) - 1) == IISAN_EWORKSPACE
    assert c.unchanged(before)
    # the reverse: a 64-wide forward (operands read 64 wide: the first T x 64 / M x 64 floats of the buffers), then a backward at 128
    c64 = _Call(lib, bs, S, 128, ws_bytes=big)
    with _lib.dev(ce_fast=4):
        _lib.check(c64.fwd(Ein=64), "iisan_inbatch_ce_fwd")
    assert (c64.tok.value >> 48) & 0xFF == 0
    before = c64.bits()
    assert c64.bwd(Ein=128) == IISAN_EBADSHAPE and b"fwd_token" in lib.iisan_last_error()
    assert c64.unchanged(before)
    # one byte short, forward
    short = _Call(lib, bs, S, 256)
    before = short.bits()
    assert short.fwd(ws_bytes=short.need - 1) == IISAN_EWORKSPACE and b"workspace" in lib.iisan_last_error()
    assert short.unchanged(before)


@pytest.mark.parametrize("bs,S", ROW_SHAPES + GENERIC_SHAPES)
def test_the_queries_without_a_width_are_the_64_wide_calls(lib, bs, S):
    for ce_fast in (1, 0, 2, 4, 3):
        with _lib.dev(ce_fast=ce_fast):
            assert lib.iisan_inbatch_ce_route_e(bs, S, 64) == lib.iisan_inbatch_ce_route(bs, S)
    assert lib.iisan_inbatch_ce_ws_bytes_e(bs, S, 64) == lib.iisan_inbatch_ce_ws_bytes(bs, S) > 0
    # no operand images at a wide width: the buffers of the f32 passes alone, of which d_prec [T, E] grows with the width
    sizes = [lib.iisan_inbatch_ce_ws_bytes_e(bs, S, E) for E in WIDTHS]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < lib.iisan_inbatch_ce_ws_bytes(bs, S)
    assert sizes[2] - sizes[0] >= 4 * bs * S * 128


@pytest.mark.parametrize("route", ["fused", "rowpass", "generic"])
def test_a_workspace_of_exactly_ws_bytes_e_is_respected_at_256(lib, route):
    """Forward + backward at E = 256, (37, 10), into a workspace of exactly `iisan_inbatch_ce_ws_bytes_e` bytes between guard zones (the
    loss and the gradients between their own): every guard byte unchanged, the result inside the bounds."""
    c = _Call(lib, 37, 10, 256)
    assert c.need > 0 and c.need % 16 == 0
    with _lib.dev(**ROUTES[route][0]):
        _lib.check(c.fwd(), "iisan_inbatch_ce_fwd")
        _lib.check(c.bwd(), "iisan_inbatch_ce_bwd")
        torch.cuda.synchronize()
    _guards_intact(c.guards())
    _check(c.loss.t.item(), c.d_score.t.cpu(), c.d_prec.t.cpu(), c.p)
