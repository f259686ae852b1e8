"""The SASRec user encoder (`iisan_sasrec_fwd/bwd`: the one-launch kernels of csrc/sasrec_fused.hip and the per-operator launches of
csrc/sasrec.hip) where a trained model and real batches put it: every other GPU test of either path feeds `x = randn` and the
`make_trainable_params` weights (scores within +-4, no sharp softmax row, no LayerNorm variance near eps, dropout 0 / 0.1, 0/1 masks with
the last position set).  Here, per regime (`_problem`):

  init        the base problem (left padding, lengths 1 .. S): the control of the rest
  sharp       w_Q, w_K x 2.5: |score| past 20, exp arguments to -50
  sharp_fwd   w_Q, w_K x 6: |score| past 100, probabilities that underflow to exact 0 (forward only)
  trained     x x 3 with channel 7 x 10, w_Q / w_K x 2.5, w_V / fc x 2, w_1 / w_2 x 3, w_1.bias x 6
  tiny        x x 1e-3, position table x 5e-3, one sequence of x exactly 0: first-LayerNorm variances at eps = 1e-6
  empty       every third sequence with an all-zero `log_mask` (the eval user without history)
  holes       `log_mask = rand > 0.4` with values 1 / 2.5 / -1: `!= 0`, not `== 1`, no left padding
  gain0       every fifth entry of every LayerNorm gain 0, the next one negated
  drop50      the base problem at dropout 0.5
  sharp_drop  `sharp` at dropout 0.1: dominant keys are dropped

on the smallest shapes that reach each one-launch instantiation and each raggedness, on both implementations (dev switch `sasrec_fused`,
the route asserted with the `sasrec_fused_fwd` counter) and on two shapes only the per-operator launches take, against `O.sasrec` in float64
on the float64 casts of the float32 inputs.  Bounds: those of
`test_gpu_trainable.py::test_sasrec_one_launch_kernels_match_the_oracle_and_the_per_operator_launches` (relative Frobenius: y 2e-5, dx and
parameter gradients 2e-5 behind the one-launch backward, 1e-3 behind the per-operator one), unchanged.  y is held row by row as well (the kernels
partition the work by rows, and one wrong row of fifty is 1/7 of its own error in the Frobenius figure of the tensor): each compared row
within 2e-5 x clamp(max |score| / 16, 1, 4).  A float32 logit carries a rounding error in proportion to its magnitude and a softmax row
passes it on one to one (dp / p = d logit), so the row-wise figure of the float32 oracle itself grows with the scores - and differs
between hosts: 1.3e-6 on one, 4.6e-6 on another for the same `sharp_fwd` problem.  Up to |score| 16 (every earlier test: at most 12) a
row gets the tensor's 2e-5; the factor stops at 4 so that 1e-4 in one row is rejected in every regime.

A query row without any allowed key (left padding, an empty sequence) carries the mask value on every key.  In float32
`score / sqrt(dh) - 1e9` is -1e9 exactly while |score / sqrt(dh)| < 32 (the spacing at 1e9 is 64): the row attends uniformly over ALL S
keys, in the kernels and in the float32 oracle.  Float64 keeps the score, so the float64 reference takes the fill -1e30, which states the
same function in that range; every problem that compares such rows asserts the range on the CPU.  Past it (`sharp`, `sharp_fwd`, `trained`)
the row is decided by rounding to multiples of 64: there y is compared on the rows that have an allowed key, and the others carry no weight
in the backward (they are padding positions: a masked key for every query) and are only held finite.

The bounds mean something because every problem asserts on the CPU (`_problem`; `test_..._are_what_they_claim` runs without a GPU) its
conditioning guard - `O.sasrec` in float32 with the reference's own -1e9 stays within 1/4 of every one-launch bound - its structure (the
regime is what it says) and its negative controls (the check rejects a slightly wrong answer, and the oracle's answer with the regime's
feature switched off).  Problems that missed one of these at first, and the seed each got instead: `RESEED`.  Measured errors:
`profiles/sasrec_regimes.md`."""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

import helpers
from iisan_amd import _lib, ops, weights
from oracle import iisan_oracle as O

L = 2
SEED = 987654321                      # of the dropout generator
REGIMES = ("init", "sharp", "sharp_fwd", "trained", "tiny", "empty", "holes", "gain0", "drop50", "sharp_drop")
OK_ROWS_ONLY = ("sharp", "sharp_fwd", "trained")          # y compared on the rows that have an allowed key
DROPOUT = {"drop50": 0.5, "sharp_drop": 0.1}
# (B, S, H, d_model).  One-launch shapes: DH 32 with four sequences per workgroup, the last workgroup holding one; DH 16, three per
# workgroup, 192 attention threads (the limit of `sasrec_fused_shape_ok`); DH 64, six per workgroup; all 48 rows of the tile, no padding
# rows; S = 1, 48 + 2 sequences.  Per-operator only: S = 20, and d_model 128 with the parameters of `test_gpu_hparams.py`.
FUSED_SHAPES = [(5, 10, 2, 64), (7, 16, 4, 64), (9, 7, 1, 64), (4, 12, 4, 64), (50, 1, 2, 64)]
PLAIN_SHAPES = [(3, 20, 2, 64), (3, 10, 4, 128)]
SHAPES = FUSED_SHAPES + PLAIN_SHAPES
# the multiplier of w_Q / w_K per regime ...
QK = {"sharp": 2.5, "sharp_drop": 2.5, "sharp_fwd": 6.0, "trained": 2.5}
# ... stepped down, and the seed offset per (regime, B, S, H, d_model): 0 unless that problem misses its structure or sits too near its
# conditioning guard (`_problem` asserts both: properties of the inputs and of the float32 / float64 oracles alone, never of the
# kernels).  The float32 oracle's sums depend on the host's BLAS and thread count - `sharp` (9, 7, 1) at offset 0: gradients 4.6e-6
# on one machine, 8.4e-6 on another - so where offset 0 left less than that factor, the first offset was taken whose float32 oracle,
# run with one thread and with eight, stays within 3e-6 of the float64 one (`trained` at S = 20: 3.3e-6, the best of ten; 2.25 instead
# of 2.5 is no better there).  The guard itself stays at 5e-6.
QK_STEP = {}                          # (no problem needed a smaller multiplier: a reseed sufficed everywhere)
RESEED = {
    # gradients at 4.6e-6 (8.4e-6 elsewhere); 3.2e-6
    ("sharp", 9, 7, 1, 64): 4, ("sharp", 4, 12, 4, 64): 1,
    # the float32 oracle's worst ROW of y at 5.5e-6, 5.2e-6, 4.2e-6, 1.3e-5, 4.8e-6 (8.3e-6 elsewhere): y as a whole is within 1.9e-6 at
    # every offset
    ("sharp_fwd", 7, 16, 4, 64): 8, ("sharp_fwd", 9, 7, 1, 64): 1, ("sharp_fwd", 4, 12, 4, 64): 2, ("sharp_fwd", 3, 20, 2, 64): 1,
    ("sharp_fwd", 3, 10, 4, 128): 5,
    # `trained` is tight against the guard: at offset 0 the float32 oracle's gradients are 3.6e-6 .. 9.9e-6 at every shape but S = 1
    ("trained", 5, 10, 2, 64): 9, ("trained", 7, 16, 4, 64): 4, ("trained", 9, 7, 1, 64): 5, ("trained", 4, 12, 4, 64): 6,
    ("trained", 3, 20, 2, 64): 8, ("trained", 3, 10, 4, 128): 4,
    # dropout at site 0 scales rows by 1 / 0.9: |score| 32.8 at offsets 0 and 1 (all rows are compared: < 32 needed) ...
    ("sharp_drop", 7, 16, 4, 64): 2,
    # ... the largest |score| of an allowed pair 19.1 / 19.0 (>= 20 needed), and gradients at 3.5e-6
    ("sharp_drop", 9, 7, 1, 64): 1, ("sharp_drop", 3, 10, 4, 128): 1, ("sharp_drop", 3, 20, 2, 64): 3,
}

PRE_A = "transformer_blocks.{}.multi_head_attention."
PRE_F = "transformer_blocks.{}.feed_forward."


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _fails(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def _base_params(S, E, g):
    """d_model 64: the user-encoder tensors of `make_trainable_params(seed=99)` (position table [10, 64]: its first S rows are read; a
    longer window draws one); d_model 128: the recipe of `test_gpu_hparams.py::_sasrec_problem`."""
    pre = "user_encoder.transformer_encoder."
    if E == 64:
        P = {k[len(pre):]: v.clone() for k, v in weights.make_trainable_params(seed=99).items() if k.startswith(pre)}
        if S > 10:
            P["position_embedding.weight"] = torch.randn(S, E, generator=g) * 0.2
        return P
    shapes = {k[len(pre):]: s for k, s in weights.trainable_shapes(emb=E, seq_len=S, n_blocks=L).items() if k.startswith(pre)}
    return weights.fill_params_seeded(shapes, seed=558)


def _drop_masks(B, S, H, E, p):
    if not p:
        return None
    masks = {0: helpers.drop_factors(SEED, 0, B * S * E, p).view(B, S, E)}
    for l in range(L):
        masks[1 + 3 * l] = helpers.drop_factors(SEED, 1 + 3 * l, B * H * S * S, p).view(B, H, S, S)
        masks[2 + 3 * l] = helpers.drop_factors(SEED, 2 + 3 * l, B * S * E, p).view(B, S, E)
        masks[3 + 3 * l] = helpers.drop_factors(SEED, 3 + 3 * l, B * S * E, p).view(B, S, E)
    return masks


def _encoder(x, lm, P, H, drop=None, fill=-1e9, eps=1e-6, masked_rows_causal=False):
    """`O.sasrec` restated with what the negative controls turn (`eps`; fully masked rows uniform over k <= q only), returning the
    intermediate values the structural assertions read.  `_problem` holds its y bit-equal to `O.sasrec`'s."""
    B, S, E = x.shape
    d = E // H
    mask = O.sasrec_mask(lm, fill)
    if masked_rows_causal:
        dead = ~((lm != 0).cumsum(1) > 0)[:, None, :, None] & ~torch.tril(torch.ones(S, S, dtype=torch.bool))[None, None]
        mask = mask.masked_fill(dead, -float("inf"))
    dr = (lambda site, t: t * drop[site]) if drop is not None else (lambda site, t: t)
    z0 = x + P["position_embedding.weight"][:S][None]
    tr = dict(var0=z0.var(-1, unbiased=False), score=[], prob=[])
    x = dr(0, F.layer_norm(z0, (E,), P["layer_norm.weight"], P["layer_norm.bias"], eps))
    for l in range(L):
        a, f = PRE_A.format(l), PRE_F.format(l)
        q = F.linear(x, P[a + "w_Q.weight"]).view(B, S, H, d).transpose(1, 2)
        k = F.linear(x, P[a + "w_K.weight"]).view(B, S, H, d).transpose(1, 2)
        v = F.linear(x, P[a + "w_V.weight"]).view(B, S, H, d).transpose(1, 2)
        sc = torch.matmul(q, k.transpose(-1, -2)) / (d ** 0.5)
        pr = torch.softmax(sc + mask, -1)
        tr["score"].append(sc)
        tr["prob"].append(pr)
        c = torch.matmul(dr(1 + 3 * l, pr), v).transpose(1, 2).reshape(B, S, E)
        x = F.layer_norm(x + dr(2 + 3 * l, F.linear(c, P[a + "fc.weight"])), (E,), P[a + "layer_norm.weight"], P[a + "layer_norm.bias"], eps)
        h = F.linear(F.relu(F.linear(x, P[f + "w_1.weight"], P[f + "w_1.bias"])), P[f + "w_2.weight"], P[f + "w_2.bias"])
        x = F.layer_norm(x + dr(3 + 3 * l, h), (E,), P[f + "layer_norm.weight"], P[f + "layer_norm.bias"], eps)
    tr["y"] = x
    return tr


def _oracle(p, dt, fill, grads=True):
    """y, dx and every parameter gradient of `O.sasrec` in `dt` on the casts of the float32 inputs; backward of (y * w).sum()."""
    Po = {k: v.to(dt).clone().requires_grad_(grads) for k, v in p["P"].items()}
    xo = p["x"].to(dt).clone().requires_grad_(grads)
    drop = None if p["masks"] is None else {s: m.to(dt) for s, m in p["masks"].items()}
    yo = O.sasrec(xo, p["lm"].to(dt), Po, p["H"], L, pre="", drop=drop, fill=fill)
    out = dict(y=yo.detach())
    if grads:
        (yo * p["w"].to(dt)).sum().backward()
        out.update(dx=xo.grad.detach(), **{k: v.grad.detach() for k, v in Po.items()})
    return out


def _errors(got, p):
    """name -> relative Frobenius error against the float64 reference (where that is exactly 0: the absolute figure); y on the compared
    rows, and 'y rows': the worst single row of them."""
    ref, cmp = p["ref"], p["cmp"].double()
    e = {}
    for k, r in ref.items():
        a = _f64(got[k])
        if k == "y":
            a, r = a * cmp[..., None], r * cmp[..., None]
            rows = (a - r).norm(dim=-1) / r.norm(dim=-1).clamp_min(1e-300)
            e["y rows"] = rows[cmp != 0].max().item()
        n = r.norm().item()
        e[k] = (a - r).norm().item() / (n or 1.0)
    return e


def _check(got, p, fused_bwd, frac=1.0):
    """The bounds of the one-launch test, times `frac` (the conditioning guard holds the float32 oracle to 1/4 of the one-launch ones)."""
    assert bool(torch.isfinite(_f64(got["y"])).all()), "y is not finite"
    e = _errors(got, p)
    bad = []
    for k, v in e.items():
        tol = 2e-5 if (fused_bwd or k == "y") else 1e-3
        if k == "y rows":
            tol = p["row_tol"]
        if k in p["ref"] and k != "y" and p["ref"][k].norm().item() == 0.0:
            tol = 1e-9
        if not v < frac * tol:
            bad.append((k, v, frac * tol))
    assert not bad, f"{len(bad)} tensors off the float64 oracle: {bad[:4]}"
    return e


@functools.lru_cache(maxsize=None)
def _problem(regime, B, S, H, E):
    """float32 x [B, S, E], log_mask [B, S], parameters and w, the dropout masks, and the float64 y, dx and parameter gradients of
    `O.sasrec` on their float64 casts - computed once per (regime, shape), shared by the routes, never modified - with the conditioning
    guard, the structural assertions and the wrong answers of the negative controls."""
    key = (regime, B, S, H, E)
    g = torch.Generator().manual_seed(zlib.crc32(f"{regime}/{B}/{S}/{H}/{E}".encode()) % (1 << 30) + RESEED.get(key, 0))
    P = _base_params(S, E, g)
    x = torch.randn(B, S, E, generator=g)
    w = torch.randn(B, S, E, generator=g)
    lengths = torch.randint(1, S + 1, (B,), generator=g)           # left padded, lengths 1 .. S, sequence 0 full, sequence 1 one item
    lengths[0] = S
    if B > 1:
        lengths[1] = 1
    lm = (torch.arange(S)[None, :] >= (S - lengths)[:, None]).float()
    qk = QK_STEP.get(key, QK.get(regime, 1.0))
    for l in range(L):
        a, f = PRE_A.format(l), PRE_F.format(l)
        P[a + "w_Q.weight"] *= qk
        P[a + "w_K.weight"] *= qk
        if regime == "trained":
            P[a + "w_V.weight"] *= 2
            P[a + "fc.weight"] *= 2
            P[f + "w_1.weight"] *= 3
            P[f + "w_2.weight"] *= 3
            P[f + "w_1.bias"] *= 6
    if regime == "trained":
        x *= 3
        x[..., 7] *= 10                                             # an outlier channel in front of the first LayerNorm
    if regime == "tiny":
        x *= 1e-3
        x[B - 1] = 0
        P["position_embedding.weight"] *= 5e-3
    if regime == "empty":
        lm[1::3] = 0                                                # the eval user whose sequence is only its target
    if regime == "holes":
        vals = torch.tensor([1.0, 2.5, -1.0])[torch.randint(0, 3, (B, S), generator=g)]
        lm = torch.where(torch.rand(B, S, generator=g) > 0.4, vals, torch.zeros(()))
        lm[:, -1] = vals[:, -1]
    P_plain = {k: v.clone() for k, v in P.items()}
    if regime == "gain0":
        for k in P:
            if k.endswith("layer_norm.weight"):
                P[k][0::5] = 0
                P[k][1::5] *= -1
    ok = (lm != 0).cumsum(1) > 0                                     # rows with at least one allowed key
    all_rows = regime not in OK_ROWS_ONLY
    cmp = torch.ones(B, S) if all_rows else ok.float()
    w = w * cmp[..., None]
    drop_p = DROPOUT.get(regime, 0.0)
    p = dict(regime=regime, B=B, S=S, H=H, E=E, P=P, x=x, lm=lm, w=w, ok=ok, cmp=cmp, drop_p=drop_p, masks=_drop_masks(B, S, H, E, drop_p),
             fwd_only=regime == "sharp_fwd", fused_shape=E == 64 and S <= 16, qk=qk)
    fill = -1e30 if all_rows else -1e9
    p["ref"] = _oracle(p, torch.float64, fill, grads=not p["fwd_only"])

    # ---- the regime is what it says (float64 oracle's own Q, K and probabilities: `_encoder` is bit-equal to `O.sasrec`)
    drop64 = None if p["masks"] is None else {s: m.double() for s, m in p["masks"].items()}
    P64 = {k: v.double() for k, v in P.items()}
    with torch.no_grad():
        tr = _encoder(x.double(), lm.double(), P64, H, drop64, fill)
        assert torch.equal(tr["y"], p["ref"]["y"]), "the restated encoder is not O.sasrec"
        tr32 = _encoder(x, lm, P, H, p["masks"])
    allowed = torch.tril((lm != 0)[:, None, None, :].expand(-1, H, S, -1))                          # [B, H, S, S]
    p["max_score"] = max(s.abs().max().item() for s in tr["score"])
    p["max_allowed"] = max(s.abs()[allowed].max().item() for s in tr["score"])
    p["row_tol"] = 2e-5 * min(4.0, max(1.0, p["max_score"] / 16))       # (module docstring)
    p["masked_rows"], p["empty_seqs"] = int((~ok).sum()), int((lm == 0).all(1).sum())
    if all_rows:
        assert p["max_score"] < 32, f"{key}: |score| {p['max_score']:.1f}: fully masked rows are not uniform in float32"
    if S > 1 and regime != "holes":
        assert p["masked_rows"] > 0, "no fully masked row"
    if regime == "empty":
        assert p["empty_seqs"] > 0 and p["empty_seqs"] < B
    else:
        assert p["empty_seqs"] == 0
    several = allowed.sum(-1) >= 2                                                                   # [B, H, S]: rows with a choice
    peak = torch.cat([pr.max(-1).values[several] for pr in tr["prob"]])
    p["peak"] = peak.median().item() if peak.numel() else float("nan")
    if regime in ("sharp", "sharp_drop") and S > 1:
        assert p["max_allowed"] >= 20, p["max_allowed"]
        # the median largest probability over the rows with at least two allowed keys, both blocks and all heads: 0.92 .. 0.98 in the
        # float64 oracle when this was written (0.34 .. 0.51 in `init`)
        assert p["peak"] >= 0.9, p["peak"]
    if regime == "sharp_fwd" and S > 1:
        assert p["max_allowed"] >= 100, p["max_allowed"]
        assert any(bool((pr[allowed] == 0).any()) for pr in tr32["prob"]), "no probability of an allowed key underflows in float32"
    if regime == "trained" and S > 1:
        assert p["max_allowed"] >= 15, p["max_allowed"]
    if regime == "tiny":
        p["min_var0"] = tr["var0"].min().item()
        assert p["min_var0"] < 2e-6, p["min_var0"]
    if regime == "holes" and S > 1:
        assert bool(((lm != 0) & (lm != 1)).any()) and bool((lm[:, :-1] == 0).any())
        assert bool(((lm == 0)[:, :-1] & (lm != 0).cumsum(1)[:, :-1].bool()).any()), "no hole behind a real position"
    if regime == "sharp_drop" and S > 1:
        hit = [bool((((pr.max(-1).values > 0.5) & several) & (p["masks"][1 + 3 * l].gather(-1, pr.argmax(-1, keepdim=True))[..., 0] == 0)).any())
               for l, pr in enumerate(tr["prob"])]
        assert any(hit), "no row whose dominant key is dropped"

    # ---- the reference is well conditioned: float32 arithmetic alone (the reference's own fill) stays within 1/4 of the one-launch bounds
    f32 = _oracle(p, torch.float32, -1e9, grads=not p["fwd_only"])
    p["floor"] = _errors(f32, p)
    try:
        _check(f32, p, True, frac=0.25)
    except AssertionError as e:
        raise AssertionError(f"an ill-conditioned reference {key}: the float32 oracle misses 1/4 of the bounds: {e}") from None

    # ---- wrong answers the check has to reject (y of the oracle with a feature switched off; the gradients are the reference's)
    def wrong_y(y):
        return dict(p["ref"], y=y)

    def enc(lm_=lm, P_=P64, drop_=drop64, **kw):
        with torch.no_grad():
            return wrong_y(_encoder(x.double(), lm_.double(), P_, H, drop_, fill, **kw)["y"])
    row = int(torch.nonzero(cmp.view(-1))[-1])
    y1 = p["ref"]["y"].clone()
    y1.view(-1, E)[row] *= 1 + 1e-4
    wrong = {"one row of y x (1 + 1e-4)": wrong_y(y1)}
    if not p["fwd_only"]:
        k0 = PRE_F.format(0) + "w_2.bias"
        wrong["d w_2.bias x (1 + 1e-4)"] = dict(p["ref"], **{k0: p["ref"][k0] * (1 + 1e-4)})
    if regime == "tiny":
        wrong["eps = 1e-5"] = enc(eps=1e-5)
    if regime == "holes" and S > 1:          # (a window of one position has one key, allowed or not: no mask changes its softmax)
        wrong["causal-only mask"] = enc(lm_=torch.ones(B, S))
        wrong["log_mask == 1"] = enc(lm_=(lm == 1).float())
    if regime in ("init", "empty") and S > 1:
        wrong["fully masked rows uniform over k <= q"] = enc(masked_rows_causal=True)
    if regime == "gain0":
        wrong["plain gains"] = enc(P_={k: v.double() for k, v in P_plain.items()})
    if regime == "drop50":
        swap = dict(drop64)
        for l in range(L):
            swap[2 + 3 * l], swap[3 + 3 * l] = drop64[3 + 3 * l], drop64[2 + 3 * l]
        wrong["masks of the neighbouring site"] = enc(drop_=swap)
    p["wrong"] = wrong
    return p


CPU_CASES = [(r,) + s for r in REGIMES for s in SHAPES]


@pytest.mark.parametrize("regime,B,S,H,E", CPU_CASES, ids=[f"{r}-{B}x{S}x{H}" + ("-d128" if E != 64 else "") for r, B, S, H, E in CPU_CASES])
def test_sasrec_regime_problems_are_what_they_claim(regime, B, S, H, E):
    """No GPU: `_problem` asserts the regime's structure and the conditioning guard; the reference passes its own check at both sets of
    bounds and every wrong answer fails it at the bound that applies to the tensor it changes."""
    p = _problem(regime, B, S, H, E)
    _check(p["ref"], p, True)
    _check(p["ref"], p, False)
    for what, got in p["wrong"].items():
        # (a gradient off by 1e-4 is what the one-launch bound rejects; the per-operator backward's 1e-3 holds its atomics' orders)
        assert _fails(_check, got, p, what.startswith("d ")), f"the bounds accept '{what}': the case does not test what it claims"


def _gpu(p, fwd_fused, bwd_fused):
    """One forward (+ backward) of `ops.SasrecFn` with the switch set per direction; the forward's route asserted from its counter."""
    order = ops.sasrec_param_order(L)
    params = [p["P"][k].cuda().requires_grad_(not p["fwd_only"]) for k in order]
    xd = p["x"].cuda().requires_grad_(not p["fwd_only"])
    cfg = ops.make_sasrec_cfg(p["S"], p["E"], p["H"], L, p["drop_p"], SEED)
    try:
        _lib.dev_set("sasrec_fused", fwd_fused)
        before = _lib.dev_get("count:sasrec_fused_fwd")
        y = ops.SasrecFn.apply(cfg, xd, p["lm"].cuda(), *params)
        one_launch = bool(fwd_fused) and p["fused_shape"]
        assert _lib.dev_get("count:sasrec_fused_fwd") == before + (1 if one_launch else 0), (fwd_fused, p["fused_shape"])
        got = dict(y=y.detach().cpu())
        if not p["fwd_only"]:
            _lib.dev_set("sasrec_fused", bwd_fused)
            (y * p["w"].cuda()).sum().backward()
            got.update(dx=xd.grad.cpu(), **{k: t.grad.cpu() for k, t in zip(order, params)})
        torch.cuda.synchronize()
    finally:
        _lib.dev_set("sasrec_fused", 1)
    return got


# (B, S, H, d_model, forward switch, backward switch): both implementations on every one-launch shape, the two mixed orders (they share
# the workspace slots) on (5, 10, 2), the per-operator-only shapes once on the default switch
GPU_CASES = [s + r for s in FUSED_SHAPES for r in ((1, 1), (0, 0))] + [FUSED_SHAPES[0] + r for r in ((1, 0), (0, 1))]
GPU_CASES += [s + (1, 1) for s in PLAIN_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H,E,fwd,bwd", GPU_CASES,
                         ids=[f"{B}x{S}x{H}" + ("-d128" if E != 64 else "") + f"-fwd{f}bwd{b}" for B, S, H, E, f, b in GPU_CASES])
@pytest.mark.parametrize("regime", REGIMES)
def test_sasrec_regimes_match_the_fp64_oracle_on_both_implementations(lib, regime, B, S, H, E, fwd, bwd):
    """`SasrecFn` against `O.sasrec` in float64: relative Frobenius 2e-5 for y (each compared row of y: 2e-5 .. 8e-5 with the largest score, module docstring), 2e-5 for dx and every
    parameter gradient behind the one-launch backward, 1e-3 behind the per-operator one; a gradient whose reference is exactly 0 (w_Q, w_K at
    S = 1) within 1e-9 absolute; y finite on the rows that are not compared."""
    p = _problem(regime, B, S, H, E)
    got = _gpu(p, fwd, bwd)
    e = _errors(got, p)
    grads = {k: v for k, v in e.items() if k not in ("y", "y rows", "dx")}
    wg = max(grads, key=grads.get) if grads else None
    floor = p["floor"]
    print(f"sasrec-regimes {regime} B={B} S={S} H={H} E={E} fwd={fwd} bwd={bwd}: y {e['y']:.2e} rows {e['y rows']:.2e}"
          + (f", dx {e['dx']:.2e}, worst gradient {grads[wg]:.2e} ({wg})" if wg else "")
          + f"; float32 oracle y {floor['y']:.1e} rows {floor['y rows']:.1e}"
          + (f" dx {floor['dx']:.1e} gradients {max(v for k, v in floor.items() if k not in ('y', 'y rows', 'dx')):.1e}" if wg else "")
          + f"; max|score| {p['max_score']:.1f} (allowed {p['max_allowed']:.1f}), peak {p['peak']:.2f}, masked rows {p['masked_rows']}")
    _check(got, p, bool(bwd) and p["fused_shape"])
