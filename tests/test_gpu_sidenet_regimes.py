"""The intra-/inter-modal side network (`iisan_side_net_fwd/bwd`: csrc/sidenet.hip, csrc/sanb.hip, the gemm32.hip epilogues and the
split-operand products of split.hip / gemm16_x3.hip) where trained taps, gates and units put it.  Every other test of it draws
`randn * 0.25` taps (iid, zero mean, one scale, independent from layer to layer), gates N(0, 0.08) (`sigmoid(theta / 0.1)` in 0.2 .. 0.8)
and adapters at std 0.05 (no unit always dead or always active, no pre-activation exactly 0).  Here, per regime (`_problem`):

  trained        per-channel means (std 0.5) and scales (0.3 .. 1.3), consecutive taps correlated 0.9, two massive channels per modality
                 (+30 / -15, one sign for every item, + 10 % per layer, 5 % jitter per item)
  massive        the massive channels at +300 / -150: |item3| in the hundreds
  gates          thetas 2.0 / -2.0 / -12.0 (saturated in float32; at -12.0 the argument of the kernels' `__expf` is 120: inf) beside
                 +-0.35 / 0.05, every tower with a shut, an open and two unsaturated gates; `remove_first` off and on
  wide_u         every fc_down.weight x 6, every fc_up.weight / 6: pre-activations past |u| = 8 (the `exp` of GELU' underflows)
  zero_u         three rows of all-zero taps and a third of step 0's fc_down.bias exactly 0: pre-activations that ARE 0 under a non-zero
                 upstream gradient (ReLU'(0) = 0, GELU'(0) = 0.5)
  dead_units     ReLU: eight units of every SANB at fc_down.bias = -1e3 (dead on every row: exactly-zero gradients), eight at +1e3
  versa_trained  asymmetric towers 256 / 512 with dim-align and a layer-drop each way, the text tap's massive channel at 2,000, fp32
                 taps and taps rounded through fp16 with `taps_exact16` (the preset-amax, no-lo-plane route)

at M = 44 (below one 64-row tile: tiled atomic weight gradients) and M = 407 (ragged 16- and 64-row tiles: split-K scratch) on every
route (`ROUTES`), through `ops.SideNetFn` on leaf tensors with the loss `(item3 * w).sum()`, against `O.side_network` /
`O.versa_side_network` in float64 on the float64 casts of the same float32 inputs.  Bounds: the existing ones (item3 2e-5; GELU gradients
5e-4 of the tensor's scale; ReLU gradients 5e-5 relative Frobenius, `test_gpu_hparams.py::_step_errors`), and, in this file only, a
tower's gate scalars held together as the vector they form in BOTH activations (GELU 2e-3 of the vector's largest entry): with
correlated taps a single gate scalar is a sum of cancelling terms and a saturated one is exactly 0 in float32.  The bounds mean something
because `test_every_problem_is_what_it_claims` asserts, without a GPU, each problem's conditioning guard (the float32 oracle within 1/4
of every bound of the float64 one), its structure and its negative controls.  Measured errors: `profiles/sidenet_regimes.md`.

Gate saturation, as measured (float32, reference and kernels alike): theta = 2.0 gives g == 1.0f and 1 - g == 0.0f, so the gate gradient
is exactly 0; theta = -12.0 gives g == 0.0f; theta = -2.0 gives 1 - g == 1.0f but g = e^-20 = 2.06e-9, NOT 0: the tap still enters with
that weight and the float64 gradient carries the factor 10 g (1 - g) = 2.06e-8, which is what `_problem` asserts for it.

Thetas stay out of 0.4 < |theta| < 1.7: there the reference's own float32 `1 - g` loses up to 2.4e-5 relative (g = 0.9975); the float32
oracle was measured 1.75e-5 off the float64 one on `cv_adapter_list.0.fc_down.bias` with theta = 0.6 in the chain - a third of the
ReLU bound before any kernel has run - and 4.6e-4, nine times the bound, with theta = 1.0 (`profiles/sidenet_regimes.md`)."""
import contextlib
import ctypes as C
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from iisan_amd import _lib, ops, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

E = 64
CACHED_HEADS = dict(cv_head="mm_encoder.cv_pre_fc.", text_head="mm_encoder.bert_pre_fc.")
COUNTERS = ("sanb_fused_fwd", "sanb_fused_bwd", "gemm32_n64f", "gemm32_k64", "gemm32_dw", "gemm_x3", "gemm_x3_group")
SATURATED, OPEN = (2.0, -2.0, -12.0), (0.35, -0.35, 0.05)
ZERO_ROWS_W = 50.0                   # zero_u: the rows of w on the all-zero items (the controls assert that this is enough)
# seed offset per problem key: 0 unless that problem's reference is ill-conditioned (`_problem` asserts it: a property of the inputs and
# of the float32 / float64 oracles alone, never of the kernels)
RESEED = {}


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _fails(check, *args, **kw):
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


def _max_err(got, want):
    return ((_f64(got) - _f64(want)).abs().max() / (_f64(want).abs().max() + 1e-300)).item()


def _fro_err(got, want):
    return ((_f64(got) - _f64(want)).norm() / (_f64(want).norm() + 1e-300)).item()


def _family(k):
    if k == "item3":
        return "item3"
    if k.startswith("gates:"):
        return "gate"
    return "adapter" if "adapter_list" in k else "fc/head"


def _errors(item3, grads, p):
    """{tensor (or "gates:<tower>", or "item3"): (error, bound)}: item3 max|err| over 2e-5 (1 + max|ref|); GELU gradients max|err| /
    max|ref| per tensor, 5e-4; ReLU gradients relative Frobenius per tensor, 5e-5; a tower's gates as the vector they form, 2e-3 of its
    largest entry (GELU) / 5e-5 Frobenius (ReLU)."""
    ref = p["g"]
    assert set(ref) <= set(grads), sorted(set(ref) - set(grads))[:4]
    a, b = _f64(item3), p["item3"]
    out = {"item3": ((a - b).abs().max().item() / (1.0 + b.abs().max().item()), 2e-5)}
    gates = {}
    gelu = p["act"] == "GELU"
    for k in ref:
        if k in p["cut"]:
            continue
        if "side_gate" in k:
            gates.setdefault(k.rsplit(".", 1)[0].rsplit("_", 1)[1], []).append(k)
        else:
            out[k] = (_max_err(grads[k], ref[k]), 5e-4) if gelu else (_fro_err(grads[k], ref[k]), 5e-5)
    for tower, ks in gates.items():
        ks = sorted(ks, key=lambda k: int(k.rsplit(".", 1)[1]))
        got, want = torch.cat([_f64(grads[k]).reshape(-1) for k in ks]), torch.cat([_f64(ref[k]).reshape(-1) for k in ks])
        out["gates:" + tower] = (_max_err(got, want), 2e-3) if gelu else (_fro_err(got, want), 5e-5)
    return out


def _check(item3, grads, p, frac=1.0):
    """Everything finite and every error within `frac` of its bound (the conditioning guard holds the float32 oracle to 1/4)."""
    assert torch.isfinite(_f64(item3)).all(), "item3 is not finite"
    for k in p["g"]:
        assert torch.isfinite(_f64(grads[k])).all(), f"the gradient of {k} is not finite"
    errs = _errors(item3, grads, p)
    bad = sorted(((e / tol, k, e) for k, (e, tol) in errs.items() if not e <= frac * tol), reverse=True)
    assert not bad, f"{len(bad)} tensors off the float64 oracle (error / bound, tensor, error): {bad[:4]}"
    return errs


def _cut_is_zero(grads, p):
    """Float32 (the kernels and the reference alike): 1 - g == 0.0f behind an open gate, so what lies before it gets exactly 0."""
    for k in p["cut"]:
        assert float(torch.as_tensor(grads[k]).abs().max()) == 0.0, f"{k} lies before an open gate: its float32 gradient is exactly 0"


def _worst(errs):
    """{family: (worst error / bound, its error, its bound)}"""
    out = {}
    for k, (e, tol) in errs.items():
        f = _family(k)
        if f not in out or e / tol > out[f][0]:
            out[f] = (e / tol, e, tol)
    return out


@contextlib.contextmanager
def _adapter_block(record=None, at_zero=None, inputs=None):
    """`O.adapter_block` restated (the same operations in the same order) so that it records the pre-activations and, for the negative
    control of `zero_u`, takes the derivative `at_zero` where a pre-activation is exactly 0."""
    real = O.adapter_block

    def block(x, P, prefix, activation="RELU"):
        h = F.linear(x, P[prefix + "fc_down.weight"], P[prefix + "fc_down.bias"])
        if record is not None:
            record[prefix] = h.detach()
        if inputs is not None:
            inputs[prefix] = x.detach()
        a = F.gelu(h) if activation == "GELU" else F.relu(h)
        if at_zero is not None:               # value + 0, derivative + (at_zero - the activation's own derivative at 0)
            own = 0.5 if activation == "GELU" else 0.0
            a = a + (at_zero - own) * torch.where(h.detach() == 0, h - h.detach(), torch.zeros_like(h))
        return F.linear(a, P[prefix + "fc_up.weight"], P[prefix + "fc_up.bias"]) + x

    O.adapter_block = block
    try:
        yield
    finally:
        O.adapter_block = real


def _trained_taps(g, M, L, D, massive):
    """[M, L, D]: channel means and scales, a shared state that moves by sqrt(1 - 0.81) randn per layer, the channels `ch` overwritten by
    the massive values."""
    mean, scale = 0.5 * torch.randn(D, generator=g), 0.3 + torch.rand(D, generator=g)
    state = torch.randn(M, D, generator=g)
    layers = []
    for l in range(L):
        if l:
            state = 0.9 * state + math.sqrt(1 - 0.81) * torch.randn(M, D, generator=g)
        layers.append(mean + scale * state)
    t = torch.stack(layers, 1).contiguous()
    ch = torch.randperm(D, generator=g)[:2]
    jitter = 1 + 0.05 * torch.randn(M, 2, generator=g)
    for j, v in enumerate(massive):
        for l in range(L):
            t[:, l, ch[j]] = v * 1.1 ** l * jitter[:, j]
    return t, ch


def _inputs(regime, act, M, kind, D, r, rm, fusion, n, exact16, seed, feature=True):
    """cfg, parameter names in ABI order, parameters, taps and w, all float32; `feature` False: the same draw with the regime's feature
    switched off (the negative control)."""
    g = torch.Generator().manual_seed(seed)
    gated, gelu = fusion == "gated", act == "GELU"
    L = 7 + int(rm)
    big = {"massive": (300.0, -150.0)}.get(regime, (30.0, -15.0))
    off = regime in ("trained", "massive", "versa_trained") and not feature
    if kind == "cached":
        dims, depth = (D, D), (L, L)
        layers = list(range(int(rm), L))
        cfg = ops.make_side_cfg(7, D, r, E, gated, gelu, rm, L, L, layers, 0)
        names = ["mm_encoder." + k for k in ops.side_param_order(7, cached=True)]
        P = weights.make_trainable_params(seed=556, cached=True, dim_cv=D, dim_text=D, down=r)
        P = {k: P[k].clone() for k in names}
        bigs = (big, big)
    else:
        dims, depth = D, n
        layers = None
        cfg = ops.make_versa_cfg(D[0], D[1], r, E, gated, gelu, False, n[0], n[1], list(range(n[0])), list(range(n[1])), taps_exact16=exact16)
        names = ["mm_encoder." + k for k in ops.versa_param_order(n[0], n[1], True)]
        P = weights.fill_params_seeded(dict(zip(names, ops.side_param_shapes(cfg))), seed=555)
        bigs = (big, (2000.0, -15.0))
    assert len(names) == len(ops.side_param_shapes(cfg)) and all(tuple(P[k].shape) == s for k, s in zip(names, ops.side_param_shapes(cfg)))
    taps, chans = [], []
    for d, l, b in zip(dims, depth, bigs):
        t, ch = _trained_taps(g, M, l, d, () if off else b)
        taps.append(t.half().float() if exact16 else t)
        chans.append(ch)
    w = torch.randn(M, 3 * E, generator=g)
    x = dict(zero_rows=None, dead=None, active=None)
    cut = []
    adapters = sorted({k.rsplit(".", 2)[0] + "." for k in names if "adapter_list" in k})
    if regime == "gates":
        for tower, nt in zip(("cv", "text", "mm"), (7, 7, 7)):
            vals = list(SATURATED) + list(OPEN) + [OPEN[int(torch.randint(0, 3, (1,), generator=g))]]
            vals = [vals[i] for i in torch.randperm(nt, generator=g).tolist()]
            # An OPEN gate in an intra-modal tower (F = g tap + (1 - g) state, 1 - g == 0.0f) cuts the state off: whatever lies before
            # it in that tower has a float64 gradient of 2e-9 of its usual size and a float32 one of exactly 0 - no relative bound
            # holds there.  So the one open gate of cv / text sits where nothing trainable lies before it (step 0), or, with
            # `remove_first` (a shut first gate passes the initial state - the first tap - through), at step 1: step 0 of those towers
            # is then `cut`, and asserted to be exactly 0 instead (`_cut_is_zero`).  The mm tower adds (F = mm + g a + (1 - g) b): no cut
            if tower != "mm":
                order = [-12.0 if tower == "cv" else -2.0, 2.0] if rm else [2.0]
                for at, v in enumerate(order):
                    i = vals.index(v)
                    vals[at], vals[i] = vals[i], vals[at]
                if rm and feature:
                    a0 = f"mm_encoder.{'cv' if tower == 'cv' else 'bert'}_adapter_list.0."
                    cut += [a0 + s for s in ("fc_down.weight", "fc_down.bias", "fc_up.weight", "fc_up.bias")]
            for k, v in enumerate(vals):
                P[f"mm_encoder.side_gate_params_{tower}.{k}"] = torch.full((1,), v if feature else 0.0)
    if regime == "wide_u" and feature:
        for a in adapters:
            P[a + "fc_down.weight"] = P[a + "fc_down.weight"] * 6
            P[a + "fc_up.weight"] = P[a + "fc_up.weight"] / 6
    if regime == "zero_u":
        x["zero_rows"] = torch.randperm(M, generator=g)[:3]
        for t in taps:
            t[x["zero_rows"]] = 0
        w[x["zero_rows"]] *= ZERO_ROWS_W
        for a in adapters:
            if a.endswith("_list.0."):
                P[a + "fc_down.bias"][0::3] = 0
    if regime == "dead_units":
        x["dead"], x["active"] = {}, {}
        for a in adapters:
            u = torch.randperm(r, generator=g)
            x["dead"][a], x["active"][a] = u[:8], u[8:16]
            if feature:
                P[a + "fc_down.bias"][u[:8]] = -1e3
                P[a + "fc_down.bias"][u[8:16]] = 1e3
                # (their activations are near 1e3: with fc_up at std 0.05 every step would add 140 to every channel of the state, the
                #  pre-activations of step 4 reach 2,000 and the dead units come alive.  Their fc_up columns x 1e-3: an ordinary unit's share)
                P[a + "fc_up.weight"][:, u[8:16]] *= 1e-3
    return dict(cfg=cfg, names=names, P=P, taps=taps, w=w, layers=layers, chans=chans, adapters=adapters, cut=cut, **x)


def _oracle(p, inp, dt, record=None, at_zero=None, grad=True, inputs=None):
    """item3 and {name: gradient} of the loss (item3 * w).sum() in `dt`."""
    Po = {k: v.detach().to(dt).clone().requires_grad_(grad) for k, v in inp["P"].items()}
    tc, tt = (t.to(dt) for t in inp["taps"])
    with _adapter_block(record, at_zero, inputs) if (record is not None or at_zero is not None) else contextlib.nullcontext():
        if p["kind"] == "cached":
            out = O.side_network(tc, tt, Po, inp["layers"], fusion=p["fusion"], activation=p["act"], remove_first=p["rm"], **CACHED_HEADS)
        else:
            out = O.versa_side_network(tc, tt, Po, list(range(p["n"][0])), list(range(p["n"][1])), fusion=p["fusion"], activation=p["act"])
        item3 = torch.cat(out, 1)
        if not grad:
            return item3.detach(), None
        (item3 * inp["w"].to(dt)).sum().backward()
    return item3.detach(), {k: v.grad.detach() for k, v in Po.items() if v.grad is not None}


def _clear_of_zero(p, inp):
    """ReLU only.  A pre-activation within float32 rounding of 0 (found: u = 1.2e-6 under a magnitude sum of 25, `gates` at M = 407) is
    a unit that one float32 evaluation order switches on and another off: ONE such element moves a [64, 768] weight gradient by 1 % of
    its Frobenius norm, 240 x the bound, on whichever route rounds the other way - a property of the inputs, which the float32 oracle's
    own rounding need not hit.  So the problem is built clear of it: step by step along the chain, a unit whose smallest non-zero |u|
    (float64) is below 64 float32 ulps of the adapter's largest sum_k |w_jk F_mk| gets its fc_down.bias entry moved by the smallest
    multiple of that margin that clears every row.  Exact zeros (`zero_u`) stay: they are exact in every evaluation order, and the
    bias entries that make them keep their value (the unit's weight on a massive channel moves instead).  Asserted
    at the end on the float32 parameters actually used."""
    steps = sorted({int(a.rsplit(".", 2)[1]) for a in inp["adapters"]})
    margin = {}
    for k in steps + [None]:
        U, X = {}, {}
        with torch.no_grad():
            _oracle(p, inp, torch.float64, record=U, grad=False, inputs=X)
        for a in inp["adapters"]:
            margin[a] = 2.0 ** -18 * (X[a].abs() @ inp["P"][a + "fc_down.weight"].double().abs().t()).max().item()
            if k is None:
                nz = U[a][U[a] != 0]
                assert nz.abs().min().item() >= 0.5 * margin[a], (a, nz.abs().min().item(), margin[a])
                continue
            if int(a.rsplit(".", 2)[1]) != k:
                continue
            for j in range(U[a].shape[1]):
                u = U[a][:, j]
                u = u[u != 0]
                if u.abs().min().item() >= margin[a]:
                    continue
                # what moves: the bias entry (every row by the same amount) - or, where `zero_u` needs that entry to stay exactly 0, the
                # unit's weight on the adapter's largest input channel (a massive one: every row in proportion to it, the all-zero rows not at all)
                live = U[a][:, j] != 0
                if p["regime"] == "zero_u" and k == 0 and j % 3 == 0:
                    c = int(X[a].abs().mean(0).argmax())
                    t, at, d = inp["P"][a + "fc_down.weight"], (j, c), X[a][live, c]
                else:
                    t, at, d = inp["P"][a + "fc_down.bias"], (j,), torch.ones_like(u)
                for i in range(1, 200):
                    s = margin[a] * (2 * ((i + 1) // 2)) * (1 if i % 2 else -1) / d.abs().mean().item()
                    new = (t[at].double() + s).float()
                    if (u + (new.double() - t[at].double()) * d).abs().min().item() >= 1.5 * margin[a]:
                        t[at] = new
                        inp["nudged"] += 1
                        break
                else:
                    raise AssertionError(f"{a} unit {j}: nothing within 200 margins clears every row")


@functools.lru_cache(maxsize=None)
def _problem(regime, act, M, kind="cached", D=768, r=64, rm=False, fusion="gated", n=(7, 7), exact16=False):
    """The float32 inputs of one side-network call, the float64 item3 and gradients of the oracle on their float64 casts - computed once
    per problem, shared by the routes, never modified - with the conditioning guard, the structural assertions (the regime is what it
    says) and the wrong answers of the negative controls."""
    key = (regime, act, M, kind, D, r, rm, fusion, n, exact16)
    seed = zlib.crc32(repr(key).encode()) % (1 << 30) + RESEED.get(key, 0)
    p = dict(regime=regime, act=act, M=M, kind=kind, D=D, r=r, rm=rm, fusion=fusion, n=n, exact16=exact16, key=key)
    inp = _inputs(*key, seed)
    inp["nudged"] = 0
    if act == "RELU":
        _clear_of_zero(p, inp)
    p.update(inp)
    p["item3"], p["g"] = _oracle(p, inp, torch.float64)
    if fusion == "gated":
        assert set(p["g"]) == set(p["names"])
    U = {}
    with torch.no_grad():
        _oracle(p, inp, torch.float64, record=U, grad=False)
    p["max_u"] = max(u.abs().max().item() for u in U.values())

    # ---- the regime is what it says
    note = {}
    for t, ch in zip(p["taps"], p["chans"]):
        mag = t.abs().mean((0, 1))
        live = torch.ones(M, dtype=torch.bool)
        if p["zero_rows"] is not None:
            live[p["zero_rows"]] = False
        cos = F.cosine_similarity(t[live, 1:].double(), t[live, :-1].double(), dim=2).mean().item()
        note.setdefault("massive/median", []).append((mag.max() / mag.median()).item())
        note.setdefault("cosine", []).append(cos)
        assert mag.max() / mag.median() >= 30 and int(mag.argmax()) in ch.tolist(), (regime, mag.max().item(), mag.median().item())
        assert cos >= 0.8, (regime, cos)
    if regime == "massive":
        assert p["item3"].abs().max().item() >= 100, p["item3"].abs().max().item()
    if regime == "gates":
        for tower in ("cv", "text", "mm"):
            ks = [k for k in p["names"] if f"side_gate_params_{tower}." in k]
            th = torch.cat([p["P"][k] for k in ks])
            g32 = torch.sigmoid(th / 0.1)
            gg = torch.cat([p["g"][k] for k in ks]).abs()
            assert bool((th == -12.0).any()) and bool((g32 == 0).any()) and bool((g32 == 1).any()), th
            assert int(((th.abs() > 0.04) & (th.abs() < 0.4)).sum()) >= 2 and not bool(((th.abs() > 0.4) & (th.abs() < 1.7)).any()), th
            assert bool((g32[th == 2.0] == 1.0).all()) and bool((g32[th == -12.0] == 0.0).all())
            # theta = -2.0: 1 - g is exactly 1 in float32, g itself is e^-20 (see the module docstring)
            assert bool(((1 - g32[th == -2.0]) == 1.0).all()) and bool((g32[th == -2.0] <= 2.0 ** -28).all())
            # float64 gradients: e^-120 at -12.0; at +-2.0 the factor 10 g (1 - g) = 2.06e-8 against >= 0.28 of an unsaturated gate, on
            # sums <dF, tap - state> of one size up to cancellation (a factor of 100 allowed for it)
            assert bool((gg[th == -12.0] <= 1e-9 * gg.max()).all()), (tower, gg)
            assert bool((gg[th.abs() == 2.0] <= 1e-5 * gg.max()).all()), (tower, gg)
            note.setdefault("saturated gate gradient / largest", []).append((gg[th.abs() >= 1.7].max() / gg.max()).item())
        assert p["P"]["mm_encoder.side_gate_params_cv.0"].item() == (-12.0 if rm else 2.0)
        assert p["P"]["mm_encoder.side_gate_params_text.0"].item() == (-2.0 if rm else 2.0) and len(p["cut"]) == (8 if rm else 0)
        for k in p["cut"]:              # float64: e^-20 of the same tensor one step on
            assert p["g"][k].norm() <= 1e-6 * p["g"][k.replace("_list.0.", "_list.1.")].norm(), k
    if regime == "wide_u":
        u0 = torch.cat([U[a].abs().reshape(-1) for a in p["adapters"] if a.endswith("_list.0.")])
        note["|u| > 8"] = (u0 > 8).double().mean().item()
        assert note["|u| > 8"] >= 0.05, note
    if regime == "zero_u":
        assert not rm
        for a in p["adapters"]:
            if a.endswith("_list.0."):
                z = U[a][p["zero_rows"]][:, 0::3]
                assert z.numel() == 3 * len(range(0, r, 3)) and bool((z == 0).all()), a
                assert bool((U[a][p["zero_rows"]][:, 1::3] != 0).all())
    if regime == "dead_units":
        for a in p["adapters"]:
            assert bool((U[a][:, p["dead"][a]] < 0).all()) and bool((U[a][:, p["active"][a]] > 0).all()), (a, p["max_u"])
    note["bias entries moved off a near-zero pre-activation"] = p["nudged"]
    p["note"] = note

    # ---- the reference is well conditioned: float32 arithmetic alone stays within 1/4 of every bound
    i32, g32_ = _oracle(p, inp, torch.float32)
    _cut_is_zero(g32_, p)
    try:
        p["floor"] = _check(i32, g32_, p, frac=0.25)
    except AssertionError as e:
        raise AssertionError(f"an ill-conditioned reference {key}: the float32 oracle misses 1/4 of the bounds: {e}") from None

    # ---- wrong answers the check has to reject
    zeroed = dict(p["g"])
    k_up = p["adapters"][len(p["adapters"]) // 2] + "fc_up.bias"
    zeroed[k_up] = torch.zeros_like(zeroed[k_up])
    wrong = {f"{k_up} gradient zeroed": (p["item3"], zeroed)}
    if regime == "zero_u":
        wrong["derivative 1 at u == 0" if act == "RELU" else "derivative 0 at u == 0"] = \
            _oracle(p, inp, torch.float64, at_zero=1.0 if act == "RELU" else 0.0)
    else:
        what = {"trained": "massive channels removed", "massive": "massive channels removed", "versa_trained": "massive channels removed",
                "gates": "gates at 0", "wide_u": "fc_down / fc_up unscaled", "dead_units": "biases as drawn"}[regime]
        wrong[what] = _oracle(p, _inputs(*key, seed, feature=False), torch.float64)
    p["wrong"] = wrong
    return p


# ---- the problems and the routes ------------------------------------------------------------------------------------------------------

def _cached_problems():
    out = []
    for M in (44, 407):
        for act in ("GELU", "RELU"):
            out += [("trained", act, M), ("massive", act, M), ("gates", act, M), ("gates", act, M, "cached", 768, 64, True),
                    ("wide_u", act, M), ("zero_u", act, M)]
        out += [("dead_units", "RELU", M), ("dead_units", "RELU", M, "cached", 768, 64, False, "sum")]
    return out


# the other `sanb_fused_ok` instantiations and the generic chain (bottleneck 32: no fused step, no n64f, no K = 64 gate epilogue)
WIDTH_PROBLEMS = [("trained", act, M, "cached", D, r) for D, r in ((256, 64), (512, 64), (1024, 64), (768, 32)) for M in (44, 407)
                  for act in ("GELU", "RELU")]
# Versa: widths 256 / 512, text deeper at M = 407 (two surplus text steps: the fused step at 512), image deeper at M = 44 (at 256)
VERSA_PROBLEMS = [("versa_trained", act, M, "versa", (256, 512), 64, False, "gated", n, x16)
                  for M, n in ((407, (5, 7)), (44, (7, 5))) for act in ("GELU", "RELU") for x16 in (False, True)]

_FUSED = dict(sanb_fused_fwd=7, sanb_fused_bwd=7, gemm32_n64f=0, gemm32_k64=1, gemm32_dw=0, gemm_x3=0, gemm_x3_group=0)
_SEPARATE = dict(sanb_fused_fwd=0, sanb_fused_bwd=0, gemm32_n64f=7, gemm32_k64=15, gemm32_dw=0, gemm_x3=0, gemm_x3_group=0)
_X3 = dict(gemm_x3=9, gemm_x3_group=3)          # the three fc layers: forward, dX, dW, a group each
# route -> (dev switches, launches of ONE forward + backward at width 768, bottleneck 64: see CACHED_CASES of test_gpu_abi_contracts.py)
ROUTES = {
    "default": ({}, _FUSED),                                                        # the fused SANB step (sanb.hip)
    "separate": (dict(sanb_fused=0), _SEPARATE),                                    # n64f, K = 64 with the gate epilogue
    "fuse_bwd": (dict(sanb_fused=0, gemm32_k64_gate=0), _SEPARATE),                 # fuse_bwd_kernel (no counter tells it from the epilogue)
    "x3": (dict(x3=2), dict(_FUSED, **_X3)),                                        # every eligible product split-operand
    "x3-separate": (dict(x3=2, sanb_fused=0), dict(_SEPARATE, **_X3)),
    "two-dw": (dict(sanb_fused=0, sidenet_dw_merge=0), _SEPARATE),                  # (the switch is the only witness: same kernels, two launches)
    "x3-fuse_bwd": (dict(x3=2, gemm32_k64_gate=0), None),                           # Versa: the aligned steps' fusion backward as its own kernel
}
CASES = [(q, route) for q in _cached_problems() for route in ("default", "separate", "fuse_bwd", "x3", "x3-separate")]
CASES += [(q, "two-dw") for q in _cached_problems() if q[2] == 407 and q[0] == "trained"]
CASES += [(q, "default") for q in WIDTH_PROBLEMS]
CASES += [(q, route) for q in VERSA_PROBLEMS for route in ("x3", "x3-separate")]
CASES += [(q, "x3-fuse_bwd") for q in VERSA_PROBLEMS if not q[9]]


def _expected_counts(p, route):
    """The launch counters that prove the route, from the host dispatch of csrc/sidenet.hip."""
    knobs, counts = ROUTES[route]
    if p["kind"] == "versa":
        # surplus steps (one tower, a supported width): fused unless switched off; the aligned steps mix widths: separate launches, whose
        # gated dF product also owes the dim-aligned tap its gradient.  Split-operand (x3 = 2): the three fc layers (9 products, 3 groups)
        # and the dim-align products with their weight gradients (2 n_mm products, 2 groups)
        n_mm, surplus = min(p["n"]), abs(p["n"][0] - p["n"][1])
        fused = surplus if knobs.get("sanb_fused", 1) else 0
        sep = n_mm + surplus - fused
        return dict(sanb_fused_fwd=fused, sanb_fused_bwd=fused, gemm32_n64f=sep, gemm32_k64=1 + 2 * sep, gemm32_dw=0,
                    gemm_x3=9 + 2 * n_mm, gemm_x3_group=5)
    if p["r"] != 64:
        return dict(_FUSED, sanb_fused_fwd=0, sanb_fused_bwd=0)
    return counts


def _id(case):
    q, route = case
    regime, act, M = q[:3]
    extra = ""
    if len(q) > 3:
        q = q + _problem.__wrapped__.__defaults__[len(q) - 3:]
        kind, D, r, rm, fusion, n, x16 = q[3:]
        extra = "".join(["-rm" if rm else "", "-sum" if fusion == "sum" else "", f"-{D}x{r}" if (kind == "cached" and (D, r) != (768, 64)) else "",
                         f"-n{n[0]}{n[1]}" if kind == "versa" else "", "-fp16taps" if x16 else ""])
    return f"{regime}{extra}-{act}-{M}-{route}"


def _counts():
    return {n: _lib.dev_get("count:" + n) for n in COUNTERS}


def _zero_counts():
    for n in COUNTERS:
        _lib.dev_set("count:" + n, 0)


def _gpu(p, route):
    """One forward + backward of `ops.SideNetFn` on leaf tensors under the route's switches.  The kernels accumulate into the leaves' own
    `.grad`, which start at 0 (`ops.DIRECT_PARAM_GRADS`, as the trainer runs them: tensors of their own, 16-byte aligned - the views of
    the one flat temporary buffer of the other path are not, and an unaligned weight gradient is no split-operand product).  Returns
    item3, {name: gradient} and the launch counters."""
    knobs = ROUTES[route][0]
    params = [p["P"][k].cuda().requires_grad_(True) for k in p["names"]]
    for t in params:
        t.grad = torch.zeros_like(t)
    tc, tt, w = p["taps"][0].cuda(), p["taps"][1].cuda(), p["w"].cuda()
    direct, flat = ops.DIRECT_PARAM_GRADS, ops._flat_grads

    def no_temporaries(params):
        raise AssertionError("the backward took temporary gradient buffers, not the leaves' .grad")

    ops.DIRECT_PARAM_GRADS, ops._flat_grads = True, no_temporaries
    try:
        with _lib.dev(**knobs):
            _zero_counts()
            item3 = ops.SideNetFn.apply(p["cfg"], tc, tt, *params)
            (item3 * w).sum().backward()
            torch.cuda.synchronize()
            counts = _counts()
    finally:
        ops.DIRECT_PARAM_GRADS, ops._flat_grads = direct, flat
        _zero_counts()
    return item3.detach().cpu(), {k: t.grad.detach().cpu() for k, t in zip(p["names"], params)}, counts


def _report(tag, p, errs):
    w, f = _worst(errs), _worst(p["floor"])
    return (f"sidenet-regimes {tag}: " + ", ".join(f"{k} {w[k][1]:.2e}/{w[k][2]:.0e} (f32 oracle {f[k][1]:.1e})" for k in sorted(w))
            + f"; max|u| {p['max_u']:.1f}, max|item3| {p['item3'].abs().max().item():.1f}")


def _controls(p):
    _check(p["item3"], p["g"], p)                                       # the reference passes its own check ...
    for what, (i3, g) in p["wrong"].items():                            # ... and every wrong answer fails it
        assert _fails(_check, i3, g, p), f"the bounds accept '{what}' {p['key']}: the problem does not test what it claims"


ALL_PROBLEMS = _cached_problems() + WIDTH_PROBLEMS + VERSA_PROBLEMS


def test_every_problem_is_what_it_claims():
    """No GPU: builds every problem, which asserts its conditioning guard and its structure (`_problem`), and runs its negative controls."""
    assert len(RESEED) <= 3 * len(ALL_PROBLEMS) and all(v <= 3 for v in RESEED.values())
    for q in ALL_PROBLEMS:
        p = _problem(*q)
        _controls(p)
        print(_report(_id((q, "float32-oracle")), p, p["floor"]), p["note"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_side_network_regimes_match_the_fp64_oracle_on_every_route(lib, case):
    """`SideNetFn` against the float64 oracle: everything finite, item3 within 2e-5, every gradient within its bound (`_errors`), the
    route proven by the launch counters; `dead_units`: the dead units' fc_down.weight rows, fc_down.bias entries and fc_up.weight columns
    EXACTLY 0 on every route (bias and gate sums leave the workgroups through float atomics; the weight gradients through atomics at
    M = 44 and the split-K scratch at M = 407)."""
    q, route = case
    p = _problem(*q)
    _controls(p)
    item3, grads, counts = _gpu(p, route)
    assert counts == _expected_counts(p, route), (route, sorted(counts.items()))
    print(_report(_id(case), p, _errors(item3, grads, p)))
    _check(item3, grads, p)
    _cut_is_zero(grads, p)
    if p["fusion"] != "gated":          # placeholders: the kernels must not write a gate gradient
        assert all(float(grads[k].abs().max()) == 0.0 for k in p["names"] if "side_gate" in k)
    if p["regime"] == "dead_units":
        for a in p["adapters"]:
            d = p["dead"][a]
            assert float(grads[a + "fc_down.weight"][d].abs().max()) == 0.0, a
            assert float(grads[a + "fc_down.bias"][d].abs().max()) == 0.0, a
            assert float(grads[a + "fc_up.weight"][:, d].abs().max()) == 0.0, a
            assert float(grads[a + "fc_down.bias"][p["active"][a]].abs().min()) > 0.0, a


@pytest.mark.gpu
@pytest.mark.parametrize("M,scratch", [(44, 0), (407, 2)])
def test_the_two_sizes_take_the_two_weight_gradient_routes(lib, M, scratch):
    """No counter tells the two apart (both are the tiled kernel, `gemm32_dw` stays 0): `iisan_gemm32_plan` on the adapters' weight-gradient
    group (dWu += dO^T A of three towers at 768 x 64, A and B stored K-major, C +=) with the split-K scratch `iisan_side_net_*` registers
    (csrc/sidenet.hip: carve).  M = 44 cannot be split: the product adds to C with atomics (plan[3] = 0); M = 407: partials through the
    scratch and the reducer's "+=" (plan[3] = 2)."""
    al = lambda x: (x + 63) // 64 * 64
    floats = max(3 * 8 * al(M * 64), 3 * 2 * 32 * al(768 * 64 + 768))
    out = (C.c_int32 * 12)()
    rc = lib.iisan_gemm32_plan((C.c_int64 * 3)(768, 768, 768), (C.c_int32 * 3)(64, 64, 64), (C.c_int64 * 3)(M, M, M), 3, 1 | 2 | 16, floats, 0, out)
    assert rc == out[0] == 0 and out[3] == scratch, tuple(out)
