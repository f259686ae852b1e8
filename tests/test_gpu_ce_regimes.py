"""The in-batch loss (`iisan_inbatch_ce_fwd/bwd`, csrc/ce.hip) where a trained model and a real batch put it: every other test of the
loss feeds it `randn * 0.3 .. 0.4` operands (logits within +-6, loss near log M), ids drawn without replacement (the false-negative mask
on one or two columns of a batch), one Zipf popularity table and clean left-padded 0/1 masks.  Here, per regime (`_problem`):

  trained    one embedding per item, prec aligned with its label's: label logits of 10 .. 30, loss 0.1 .. 3
  sharp      logits to +-75, loss 30 .. 45: exp arguments down to -150
  ramp       score rows growing along the walk: the running maximum moves in every wave and every Y range up to the last tile
  outlier    every 7th score row x 8: the per-tensor amax scale of the split planes, most rows at 1/8 of it
  repeats    ids redrawn WITH replacement from 12 items (`repeats`: the mask on a fifth of the columns and more, the label's id again in
             its own sequence) and from 5 (`repeats5`; min(5, S) where S < 5: the mask on most columns, and rows left without any
             negative - a row loses them all only if its sequence holds every id of the batch, which twelve ids cannot in six slots,
             so sequence 0 of `repeats5` is full length and is given the whole catalogue)
  one_item   a catalogue of one item: every negative masked, loss and gradients exactly 0
  wide_pop   popularities over seven decades: debias terms up to +18 on sharp logits
  holes      `log_mask` with holes and values 2.5 / -1 on unchanged ids: column padding by `log_mask` alone, `!= 0` not `== 1`, label
             columns that are themselves padding (their logit is the fill value; no gradient flows through a filled logit)

on the four row-fixed instantiations' smallest shapes x every route (`ce_fast` 4 / 2 / 0 / 3, `ce16_nsub`, `ce16_ys`; the default knobs
once) and on three generic-only shapes, against `O.inbatch_ce` in float64 on the same float32 inputs.  Bounds: those of
`test_gpu_hparams.py::_check_ce` and the ragged split-operand test (loss 2e-5 relative, gradients 2e-4 of their scale + 1e-9), unchanged.
They mean something here because every problem carries a conditioning guard asserted on the CPU - `O.inbatch_ce` in float32 stays within
1/8 of each bound of the float64 result, and the float64 loss is >= 0.1 - its structural assertions (the regime is what it says) and its
negative controls (the check rejects a slightly wrong answer, and the answer of the oracle with the regime's feature switched off).
Measured errors: `profiles/ce_regimes.md`."""
import functools
import random
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from iisan_amd import _lib, ops, synth  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

E = 64
MASKV = -1e4
REGIMES = ("trained", "sharp", "ramp", "outlier", "repeats", "repeats5", "one_item", "wide_pop", "holes")
TRAINED_FAMILY = ("trained", "repeats", "repeats5", "one_item", "wide_pop", "holes")
CATALOGUE = {"repeats": 12, "repeats5": 5, "one_item": 1}
# prec = a * unit(score[label]) + 0.3 N(0, 1): the first a of this list whose float64 loss is >= 0.1 (`trained` itself: in [0.1, 3])
ALIGN = (1.5, 1.25, 1.0, 0.75, 0.5, 0.35, 0.25)
# seed offset per (regime, bs, S): 0 unless that problem's reference is ill-conditioned or its structure is not the regime's (`_problem`
# asserts both; a property of the inputs and the float32 / float64 oracles alone, never of the kernels)
RESEED = {("repeats5", 5, 31): 2}       # (0: every sequence holds all five items, loss 0; 1: loss 0.03 at the smallest a)

ROW_SHAPES = [(7, 5), (37, 10), (6, 15), (64, 10)]
GENERIC_SHAPES = [(9, 3), (4, 16), (5, 31)]
# route name -> (dev switches, iisan_inbatch_ce_route's answer on a row-fixed shape)
ROUTES = {
    "default": ({}, 2),                                        # < 2^24 logits: the fused f32 row pass
    "fused": (dict(ce_fast=4), 2),
    "rowpass": (dict(ce_fast=2), 1),
    "generic": (dict(ce_fast=0), 0),
    "ce16": (dict(ce_fast=3, ce16_nsub=1, ce16_ys=0), 3),
    "ce16_nsub2": (dict(ce_fast=3, ce16_nsub=2, ce16_ys=0), 3),
    "ce16_ys16": (dict(ce_fast=3, ce16_nsub=1, ce16_ys=16), 3),    # sixteen Y ranges on 12 / 13 steps: empty ranges
}
CASES = [(bs, S, r) for bs, S in ROW_SHAPES for r in ("default", "fused", "rowpass", "generic", "ce16")]
CASES += [(37, 10, "ce16_nsub2"), (37, 10, "ce16_ys16")]
CASES += [(bs, S, "default") for bs, S in GENERIC_SHAPES]


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _close(a, b, rtol, atol, what):
    a, b = _f64(a), _f64(b)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max|err| {err:.3e} vs scale {ref:.3e}"


def _fails(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def _errors(loss, d_score, d_prec, p):
    """(|loss - loss64| / |loss64|, max|d_score - ref| / max|ref|, the same of d_prec); where the reference is exactly 0 the absolute figure."""
    el = abs(float(loss) - p["loss"]) / (abs(p["loss"]) or 1.0)
    eg = [((_f64(g) - w).abs().max() / (w.abs().max().item() or 1.0)).item() for g, w in ((d_score, p["d_score"]), (d_prec, p["d_prec"]))]
    return el, eg[0], eg[1]


def _check(loss, d_score, d_prec, p, frac=1.0):
    """The bounds of `test_gpu_hparams.py::_check_ce`, times `frac` (the conditioning guard holds the float32 oracle to 1/8 of them)."""
    assert np.isfinite(float(loss)), loss
    if p["regime"] == "one_item":       # the float64 loss is exactly 0: lse and the label logit are two float32 roundings of one quantity
        assert abs(float(loss)) <= frac * 8 * 2.0 ** -24 * p["max_logit"], (float(loss), p["max_logit"])
        for what, g in (("d_score", d_score), ("d_prec", d_prec)):
            assert torch.isfinite(_f64(g)).all() and _f64(g).abs().max().item() <= frac * 1e-9, (what, _f64(g).abs().max().item())
        return
    assert abs(float(loss) - p["loss"]) <= frac * 2e-5 * abs(p["loss"]), (float(loss), p["loss"])
    _close(d_score, p["d_score"], frac * 2e-4, frac * 1e-9, "d_score")
    _close(d_prec, p["d_prec"], frac * 2e-4, frac * 1e-9, "d_prec")


def _oracle(ids, score, prec, log_mask, pop, dt):
    so, po = score.detach().to(dt).clone().requires_grad_(True), prec.detach().to(dt).clone().requires_grad_(True)
    loss = O.inbatch_ce(ids, so, po, log_mask.to(dt), pop.to(dt))
    loss.backward()
    return loss.item(), so.grad.detach(), po.grad.detach()


def _left_padding(ids):
    return (ids[:, :-1] != 0).float()


@functools.lru_cache(maxsize=None)
def _problem(regime, bs, S):
    """ids [bs, S + 1], log_mask [bs, S], pop_prob, score [bs (S + 1), 64] and prec [bs S, 64] in float32, the float64 loss and gradients
    of `O.inbatch_ce` on their float64 casts - computed once per (regime, bs, S), shared by the routes, never modified - with the
    conditioning guard, the structural assertions and the wrong answers of the negative controls."""
    seed = zlib.crc32(f"{regime}/{bs}/{S}".encode()) % (1 << 30) + RESEED.get((regime, bs, S), 0)
    rnd = random.Random(seed)
    lengths = [rnd.randint(2, S + 1) for _ in range(bs)]            # ragged, as `test_gpu_hparams.py::_ce_problem`
    if regime == "repeats5":
        lengths[0] = S + 1                                           # (one full sequence: it is given the whole catalogue below)
    n = max(40, bs * 3, 2 * (S + 1))
    rs = np.random.RandomState(seed)
    ids, log_mask = synth.make_ids(bs, S, n, rs, lengths)            # left padded with id 0
    if regime in CATALOGUE:
        # (a row loses every negative only if its sequence holds every id of the batch: five items do not fit the four slots of S = 3)
        cat = min(CATALOGUE[regime], S) if regime == "repeats5" else CATALOGUE[regime]
        real = ids != 0
        ids[real] = rs.randint(1, cat + 1, size=int(real.sum()))
        if regime == "repeats5":                                     # sequence 0 holds every item, and (S + 1 > cat slots) one of them twice
            ids[0, S + 1 - cat:] = 1 + rs.permutation(cat)
    ids, log_mask = torch.from_numpy(ids), torch.from_numpy(log_mask)
    pop = synth.make_pop_prob(n)
    g = torch.Generator().manual_seed(seed)
    T, M = bs * S, bs * (S + 1)
    label = (torch.arange(bs)[:, None] * (S + 1) + torch.arange(1, S + 1)[None, :]).view(-1)
    if regime == "wide_pop":
        pop = torch.cat([torch.ones(1), 10.0 ** (-1 - 7 * torch.rand(n, generator=g))])
    if regime == "holes":
        on = torch.rand(bs, S, generator=g) < 0.6
        vals = torch.tensor([1.0, 2.5, -1.0])[torch.randint(0, 3, (bs, S), generator=g)]
        log_mask = torch.where(on, vals, torch.zeros(()))
        log_mask[:, -1] = vals[:, -1]

    align = None
    if regime in TRAINED_FAMILY:
        emb = torch.randn(n + 1, E, generator=g)
        score = emb[ids.view(-1)]                                    # one embedding per item id, as the model produces it
        unit = score[label] / score[label].norm(dim=1, keepdim=True)
        noise = 0.3 * torch.randn(T, E, generator=g)
        for align in ALIGN:
            prec = align * unit + noise
            with torch.no_grad():
                l64 = O.inbatch_ce(ids, score.double(), prec.double(), log_mask.double(), pop.double()).item()
            if l64 >= 0.1 or regime == "one_item":
                break
    elif regime == "sharp":
        score, prec = 2 * torch.randn(M, E, generator=g), torch.randn(T, E, generator=g)
    elif regime == "ramp":
        score = torch.randn(M, E, generator=g) * (0.25 + 1.75 * torch.arange(M) / (M - 1))[:, None]
        prec = torch.randn(T, E, generator=g)
    elif regime == "outlier":
        score, prec = 0.5 * torch.randn(M, E, generator=g), torch.randn(T, E, generator=g)
        score[::7] *= 8
    else:
        raise KeyError(regime)

    loss, ds, dp = _oracle(ids, score, prec, log_mask, pop, torch.float64)
    with torch.no_grad():
        z, lab = O.inbatch_logits(ids, score.double(), prec.double(), log_mask.double(), pop.double())
    assert torch.equal(lab, label)
    valid = log_mask.reshape(-1) != 0
    live = z != MASKV
    p = dict(regime=regime, bs=bs, S=S, ids=ids, log_mask=log_mask, pop=pop, score=score, prec=prec, loss=loss, d_score=ds, d_prec=dp,
             align=align, max_logit=z[live].abs().max().item())

    # ---- the regime is what it says
    col_pad = torch.cat([log_mask, torch.ones(bs, 1)], 1).view(-1) == 0
    neg = live.clone()
    neg[torch.arange(T), label] = False
    no_negative = valid & ~neg.any(1)
    if regime in ("repeats", "repeats5"):
        seq = ids.view(bs, S + 1)
        twice = (seq[:, None, 1:] == seq[:, :, None]).sum(1) >= 2                         # [bs, S]: the label's id occurs again in its sequence
        if regime == "repeats5":
            assert bool(no_negative.any()), "no valid row is left without a negative"
        fired = (z == MASKV) & ~col_pad[None, :]                                          # filled by the false-negative rule alone
        p["masked"] = fired[valid].double().mean().item() / (~col_pad).double().mean().item()
        assert p["masked"] >= (0.5 if regime == "repeats5" else 0.2), p["masked"]
        assert bool((twice.reshape(-1) & valid).any()), "no valid row's label id occurs twice in its sequence"
    if regime == "one_item":
        assert bool(no_negative[valid].all()) and bool(valid.any())
        assert loss == 0.0 and float(ds.abs().max()) == 0.0 and float(dp.abs().max()) == 0.0
    if regime == "ramp":
        # the largest live logit of at least half the valid rows sits at a column c >= M - max(16, M / 4): in the last quarter of the
        # columns (behind three quarters of every wave's round-robin walk, in the last ce16 Y ranges) or, where that quarter is shorter
        # than a tile, in the last 16 columns - and the scale of the logits grows along the whole walk
        late = z.masked_fill(~live, -float("inf")).argmax(1) >= M - max(16, M // 4)
        assert int((late & valid).sum()) * 2 >= int(valid.sum()), (int((late & valid).sum()), int(valid.sum()))
    if regime == "sharp":
        assert p["max_logit"] >= 50, p["max_logit"]
    if regime == "holes":
        lab_pad = col_pad[label]
        assert bool((lab_pad & valid).any()), "no valid row's label column is padding"
        assert bool(((log_mask != 0) & (log_mask != 1)).any()) and not torch.equal(log_mask != 0, _left_padding(ids) != 0)
    if regime == "trained":
        assert 0.1 <= loss <= 3.0, loss
    if regime != "one_item":
        assert loss >= 0.1, loss

    # ---- the reference is well conditioned: float32 arithmetic alone stays within 1/8 of every bound
    l32, ds32, dp32 = _oracle(ids, score, prec, log_mask, pop, torch.float32)
    p["floor"] = _errors(l32, ds32, dp32, p)
    try:
        _check(l32, ds32, dp32, p, frac=0.125)
    except AssertionError as e:
        raise AssertionError(f"an ill-conditioned reference ({regime}, {bs}, {S}): the float32 oracle misses 1/8 of the bounds: {e}") from None

    # ---- wrong answers the check has to reject
    wrong = {"loss x (1 + 1e-4)": (loss * (1 + 1e-4), ds, dp)}
    zeroed = ds.clone()
    zeroed[int(ds.abs().max(1).values.argmax())] = 0
    wrong["largest d_score row zeroed"] = (loss, zeroed, dp)
    if regime == "one_item":
        wrong = {"loss of 16 ulps": (16 * 2.0 ** -24 * p["max_logit"], ds, dp), "d_prec of 2e-9": (0.0, ds, dp + 2e-9)}
    if regime in ("repeats", "repeats5"):        # ids made distinct (the column index), popularities carried along: no false-negative mask
        wrong["no false-negative mask"] = _oracle(torch.arange(M).view(bs, S + 1), score, prec, log_mask, pop[ids.view(-1)], torch.float64)
    if regime == "wide_pop":
        wrong["uniform pop_prob"] = _oracle(ids, score, prec, log_mask, torch.full_like(pop, 1.0 / n), torch.float64)
    if regime == "holes":
        wrong["left-padding log_mask"] = _oracle(ids, score, prec, _left_padding(ids), pop, torch.float64)
    p["wrong"] = wrong
    return p


def _gpu(lib, p, route):
    """One forward + backward of `ops.InbatchCeFn` on the route's switches; the route and the ce16 counter asserted while they are set."""
    bs, S = p["bs"], p["S"]
    knobs, want = ROUTES[route]
    if S < 5 or S >= 16:
        want = 0
    sd, pd = p["score"].cuda().requires_grad_(True), p["prec"].cuda().requires_grad_(True)
    ids, lm, pop = p["ids"].view(-1).cuda(), p["log_mask"].cuda(), p["pop"].cuda()
    with _lib.dev(**knobs):
        assert lib.iisan_inbatch_ce_route(bs, S) == want, (route, lib.iisan_inbatch_ce_route(bs, S), want)
        before = _lib.dev_get("count:ce16")
        loss = ops.InbatchCeFn.apply(ids, sd, pd, lm, pop)
        loss.backward()
        torch.cuda.synchronize()
        assert _lib.dev_get("count:ce16") == before + (1 if want == 3 else 0)
    return loss.item(), sd.grad.cpu(), pd.grad.cpu(), want


@pytest.mark.parametrize("bs,S,route", CASES, ids=[f"{bs}x{S}-{r}" for bs, S, r in CASES])
@pytest.mark.parametrize("regime", REGIMES)
def test_inbatch_ce_regimes_match_the_fp64_oracle_on_every_route(lib, regime, bs, S, route):
    """`InbatchCeFn` against `O.inbatch_ce` in float64: loss within 2e-5 relative, d_score and d_prec within 2e-4 of their scale + 1e-9
    (`one_item`, whose reference is exactly 0: |loss| <= 8 x 2^-24 x max|logit|, gradients <= 1e-9).  Shapes: (7, 5) three Y tiles (one
    wave gets none, the last partial, a 16-row block over four sequences); (37, 10) RS1 = 11 with a partial last tile; (6, 15) RS1 = 16,
    whole tiles; (64, 10) whole 32-row ce16 steps; (9, 3), (4, 16), (5, 31) the generic kernel on default switches."""
    p = _problem(regime, bs, S)
    _check(p["loss"], p["d_score"], p["d_prec"], p)                     # the reference passes its own check ...
    for what, (l, ds, dp) in p["wrong"].items():                        # ... and every wrong answer fails it
        assert _fails(_check, l, ds, dp, p), f"the bounds accept '{what}': the case does not test what it claims"
    loss, ds, dp, want = _gpu(lib, p, route)
    el, es, ep = _errors(loss, ds, dp, p)
    print(f"ce-regimes {regime} bs={bs} S={S} route={route}({want}): loss {p['loss']:.4g} err {el:.2e}, d_score {es:.2e}, d_prec {ep:.2e}, "
          f"max|logit| {p['max_logit']:.1f}; float32 oracle {p['floor'][0]:.1e} / {p['floor'][1]:.1e} / {p['floor'][2]:.1e}"
          + (f", a = {p['align']}" if p["align"] else ""))
    _check(loss, ds, dp, p)
