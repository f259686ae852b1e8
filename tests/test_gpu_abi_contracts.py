"""The written promises of the trainable C ABI (`include/iisan_hip.h`) that the product's own Python never exercises:

  A. parameter gradients ACCUMULATE (`+=`): every backward entry point and kernel route started from NON-ZERO gradient tensors
     (`ops.DIRECT_PARAM_GRADS`: the kernels write into `p.grad` itself), expected `G0 + g_oracle`, twice in a row `G0 + 2 g_oracle`;
  B. `iisan_linear_fwd` / `iisan_linear_bwd` called directly, "dx / dw / db may be NULL to skip" included;
  C. `d_loss` of `iisan_inbatch_ce_bwd` is a plain multiplier on all four loss routes, and the backward leaves the workspace as the
     forward filled it;
  D. `*_ws_bytes()` is sufficient AND respected (guard zones around the workspace and every output), one byte less is
     `IISAN_EWORKSPACE` before anything is launched, `fwd_token = 0` is `IISAN_EBADSHAPE`.

References are the CPU oracle (`oracle/iisan_oracle.py`, fp32 as in the route tests of `test_gpu_trainable.py`, fp64 for the loss and
the Linear layer); bounds are the ones those tests already hold the same tensors to.  Every accumulation test carries its negative
control: the comparison that accepts `G0 + g` must reject `g` alone (an overwriting kernel) and `G0 + 2 g` (a double add)."""
import contextlib
import ctypes as C
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
from iisan_amd import _lib, ops, synth, tapstore, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

IISAN_EBADSHAPE, IISAN_EWORKSPACE = -1, -2
GUARD, GUARD_BYTE = 4096, 0xA5
CACHED_HEADS = dict(cv_head="mm_encoder.cv_pre_fc.", text_head="mm_encoder.bert_pre_fc.")
COUNTERS = ("sanb_fused_fwd", "sanb_fused_bwd", "gemm32_n64f", "gemm32_k64", "gemm32_dw", "gemm_x3", "gemm_x3_group", "sasrec_fused_fwd")
# iisan_gemm32_plan: flags of a weight-gradient product (A and B stored K-major, C +=) and the plan fields asserted below
G32_DW = 1 | 2 | 16
PLAN_TILED, PLAN_DW = 0, 2                      # plan12[0]: kernel
SCRATCH_NONE, SCRATCH_ADD_C = 0, 2              # plan12[3]: "+=" by atomics in the product / partials through the scratch + reducer
COLSUM_NONE, COLSUM_FOLDED, COLSUM_OWN = 0, 1, 2    # plan12[6]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _close(a, b, rtol, atol, what):
    """The comparison of `test_gpu_trainable.py::test_gemm32_vs_torch`."""
    a, b = _f64(a), _f64(b)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max|err| {err:.3e} vs scale {ref:.3e}"


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _max_err(got, want, g):
    """max|got - want| / max|g|: the per-tensor figure of the route tests (GELU adapters)."""
    return ((_f64(got) - _f64(want)).abs().max() / (_f64(g).abs().max() + 1e-300)).item()


def _fro_err(got, want, g):
    """|got - want| / |g| in the Frobenius norm: the figure of the SASRec one-launch test."""
    return ((_f64(got) - _f64(want)).norm() / (_f64(g).norm() + 1e-300)).item()


def _route_tol(name):
    return 2e-3 if ("user_encoder" in name or "side_gate" in name) else 5e-4


def _draw_g0(g, seed):
    """Per tensor, uniform in [-s, s] with s = max|g| of that tensor: an overwrite is then an error of order s.  (A ONE-element tensor - a
    gate - draws |G0| below bound x s with a probability equal to the bound; the seeds are fixed, and the negative controls assert that
    none did.)"""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k in sorted(g):
        s = g[k].abs().max().item()
        out[k] = ((torch.rand(g[k].shape, generator=gen) * 2 - 1) * s).float()
    return out


def _errors(got, G0, g, a, b, err_fn):
    """{name: err_fn(got, a G0 + b g, g)}"""
    return {k: err_fn(got[k], a * G0[k].double() + b * g[k].double(), g[k]) for k in g}


def _assert_accumulated(got, G0, g, times, err_fn, tol_of, what):
    """Positive assertion: every tensor within its bound of G0 + times * g.  Returns (worst err / tol, its name, its err)."""
    errs = _errors(got, G0, g, 1, times, err_fn)
    bad = sorted(((e, k) for k, e in errs.items() if not e < tol_of(k)), reverse=True)
    assert not bad, f"{what}: {len(bad)} tensors off G0 + {times} g: {bad[:4]}"
    e, k = max((e / tol_of(k), k) for k, e in errs.items())
    return e, k, errs[k]


def _assert_rejected(got, G0, g, a, b, err_fn, tol_of, what):
    """Negative control, same comparison: NO tensor may pass against a G0 + b g."""
    errs = _errors(got, G0, g, a, b, err_fn)
    passed = sorted(k for k, e in errs.items() if e < tol_of(k))
    assert not passed, f"{what}: the comparison would accept {passed[:4]} ({len(passed)} tensors) - G0 too small for the bound to mean anything"


def _accumulation_checks(runs, G0, g, err_fn, tol_of, what):
    """`runs` = gradients after the first and after the second backward.  Positive, both negative controls, second backward."""
    w1 = _assert_accumulated(runs[0], G0, g, 1, err_fn, tol_of, what + " (first backward)")
    _assert_rejected(runs[0], G0, g, 0, 1, err_fn, tol_of, what + " against g alone (an overwrite)")
    _assert_rejected(runs[0], G0, g, 1, 2, err_fn, tol_of, what + " against G0 + 2 g (a double add)")
    w2 = _assert_accumulated(runs[1], G0, g, 2, err_fn, tol_of, what + " (second backward, no zeroing)")
    print(f"abi-contracts {what}: worst err/bound {w1[0]:.3f} ({w1[1]} {w1[2]:.2e}); second backward {w2[0]:.3f} ({w2[1]} {w2[2]:.2e})")


@contextlib.contextmanager
def _direct_param_grads():
    """`ops.DIRECT_PARAM_GRADS = True`, and the zeroed temporaries of the plain route made an error: `_grad_targets` falls back to them
    silently when a `p.grad` is unusable, and AccumulateGrad would then add into G0 for the kernels."""
    old, flat = ops.DIRECT_PARAM_GRADS, ops._flat_grads

    def no_temporaries(params):
        raise AssertionError("the backward took zeroed temporary gradient buffers, not p.grad")

    ops.DIRECT_PARAM_GRADS, ops._flat_grads = True, no_temporaries
    try:
        yield
    finally:
        ops.DIRECT_PARAM_GRADS, ops._flat_grads = old, flat


def _counts():
    return {n: _lib.dev_get("count:" + n) for n in COUNTERS}


def _zero_counts():
    for n in COUNTERS:
        _lib.dev_set("count:" + n, 0)


def _plan(lib, probs, flags, scratch_floats, with_colsum):
    n = len(probs)
    out = (C.c_int32 * 12)()
    rc = lib.iisan_gemm32_plan((C.c_int64 * n)(*[q[0] for q in probs]), (C.c_int32 * n)(*[q[1] for q in probs]),
                               (C.c_int64 * n)(*[q[2] for q in probs]), n, flags, scratch_floats, with_colsum, out)
    assert rc == out[0]
    return tuple(out)


def _side_scratch_floats(M, dims, r=64):
    """The split-K scratch `iisan_side_net_*` registers for its products (csrc/sidenet.hip: carve)."""
    al = lambda x: (x + 63) // 64 * 64
    return max(3 * 8 * al(M * r), sum(2 * 32 * al(d * r + d) for d in dims))


# =====================================================================================================================================
# A. accumulation into non-zero gradients
# =====================================================================================================================================

@functools.lru_cache(maxsize=None)
def _cached_reference(bs, fusion="gated"):
    """Cached model, 7 taps x 768, n = 500 items, S = 10, GELU adapters: batch, parameters, tap tables, the oracle's loss and gradients
    (computed once per batch size, shared by the cases of that size, never modified) and the G0 drawn from them.
    The oracle runs in fp64 AND in fp32, and the two must agree to 1e-4 of every tensor's scale.  A gate gradient is ONE scalar, a sum of
    cancelling <dF, tap - state> products, held to 2e-3 OF ITSELF: where a batch happens to cancel it to 1/1000 of its neighbours
    (batch seed 43 at bs = 4: gate cv.2 is -3.8e-4 beside -0.30 and -0.85; seed 46 at bs = 64: text.6) the fp32 oracle itself is 1.5e-3
    .. 4.7e-2 off the fp64 one and the bound measures that batch's conditioning, not a kernel.  Batch seed 45 is the first from 43 on
    whose four batch sizes are free of such a scalar (worst fp32-vs-fp64 4.3e-5) - a property of the reference alone, asserted here."""
    n = 500
    b = synth.scientific_batch(bs=bs, seed=45, item_num=n, res=2, words=2)
    P = weights.make_trainable_params(seed=556, cached=True)
    if fusion != "gated":
        P = {k: v for k, v in P.items() if "side_gate" not in k}
    g = torch.Generator().manual_seed(5)
    tabs = [torch.randn(n + 1, 7, 768, generator=g) * 0.25 for _ in range(2)]
    for t in tabs:
        t[0] = 0                                   # the padding item (TapStore zeroes that row too)
    ids = b.ids.view(-1)
    out = {}
    for dt in (torch.float32, torch.float64):
        Po = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in P.items()}
        loss, _ = O.model_loss_from_taps(ids, tabs[0][ids].to(dt), tabs[1][ids].to(dt), b.log_mask.to(dt), b.pop_prob.to(dt), Po,
                                         list(range(7)), activation="GELU", fusion=fusion, **CACHED_HEADS)
        loss.backward()
        out[dt] = (loss.item(), {k: v.grad.detach() for k, v in Po.items()})
    loss, grads = out[torch.float64]
    own = max((_max_err(out[torch.float32][1][k], grads[k], grads[k]), k) for k in grads)
    assert own[0] < 1e-4, f"an ill-conditioned reference (fp32 oracle vs fp64 oracle {own}): choose another batch"
    return dict(b=b, P=P, tabs=tabs, loss=loss, g=grads, G0=_draw_g0(grads, seed=1000 + bs))


def _cached_two_backwards(bs, knobs, fusion="gated"):
    """The real call path: p.grad = G0 on every trainable parameter, DIRECT_PARAM_GRADS, loss.backward() - twice, each on a fresh forward,
    without zeroing.  Returns (reference, [gradients after backward 1, after backward 2], launch counters of ONE forward + backward)."""
    ref = _cached_reference(bs, fusion)
    b = ref["b"]
    args = helpers.make_args(drop_rate=0.0, adapter_activation="GELU", fusion_method=fusion)
    model = helpers.build_model(args, 500, b.pop_prob, cached=True)
    helpers.load_trainables(model, ref["P"])
    model.tap_stores = tuple(tapstore.TapStore(t.cuda(), range(7), "cuda", "fp32") for t in ref["tabs"])
    model.train()
    named = {k: p for k, p in model.named_parameters() if p.requires_grad}
    assert set(named) == set(ref["g"]) and len(named) == (146 if fusion == "gated" else 125)
    for k, p in named.items():
        p.grad = ref["G0"][k].cuda().clone()
    ids, lm = b.ids.view(-1).cuda(), b.log_mask.cuda()
    runs, counts = [], None
    with _lib.dev(**knobs), _direct_param_grads():
        for _ in range(2):
            _zero_counts()
            loss = model(ids, None, None, lm, None)
            loss.backward()
            torch.cuda.synchronize()
            counts = _counts()
            assert abs(loss.item() - ref["loss"]) <= 2e-5 * abs(ref["loss"]), (loss.item(), ref["loss"])
            runs.append({k: p.grad.detach().cpu().clone() for k, p in named.items()})
    _zero_counts()
    return ref, runs, counts, model


# Launches of ONE Cached forward + backward (7 SANB steps) by kernel family, as the host dispatch of csrc/sidenet.hip makes them:
#   fused SANB steps (below SANB_FUSED_MAX_ROWS = 4,096 item slots): 7 + 7 fused launches; the one K = 64 product left is dY = dE Wh;
#   separate launches: 7 fusion-fed down projections, K = 64 kernel 7 (up projections) + 1 (dY) + 7 (dF, with or without the gate epilogue).
_FUSED = dict(sanb_fused_fwd=7, sanb_fused_bwd=7, gemm32_n64f=0, gemm32_k64=1, gemm_x3=0, gemm_x3_group=0, sasrec_fused_fwd=1)
_SEPARATE = dict(sanb_fused_fwd=0, sanb_fused_bwd=0, gemm32_n64f=7, gemm32_k64=15, gemm_x3=0, gemm_x3_group=0, sasrec_fused_fwd=1)
_W3 = lambda M: [(768, 64, M)] * 3                 # dWu += dO^T A of the three towers (weight-gradient layout: M x N x K)
_W6 = lambda M: _W3(M) + [(64, 768, M)] * 3        # ... and dWd += dU^T F in the same launch
CACHED_CASES = {
    # 44 slots, product default: fused SANB steps (sanb.hip bias / gate atomics); K = 44 cannot be split: the tiled kernel adds to C with
    # atomics (adapters, heads, fc); colsum_kernel for the head / fc biases
    "bs4": dict(bs=4, knobs={}, counts=dict(_FUSED, gemm32_dw=0), group=_W3, colsum=0, plan=(PLAN_TILED, SCRATCH_NONE, COLSUM_NONE)),
    # 44 slots never take the separate launches by themselves (the fused step serves every size below 4,096): switched, with the gate
    # epilogue off - fuse_bwd_kernel's gate atomic (sidenet.hip), the tiled atomic kernel on six problems, colsum_kernel for dbu / dbd
    "bs4-separate": dict(bs=4, knobs=dict(sanb_fused=0, gemm32_k64_gate=0), counts=dict(_SEPARATE, gemm32_dw=0), group=_W6, colsum=1,
                         plan=(PLAN_TILED, SCRATCH_NONE, COLSUM_OWN)),
    # 407 slots (no multiple of 64): split-K partials through the scratch + gemm32_reduce_kernel's ADD_C behind the TILED kernel
    # (the plan says scratch, not atomics), ragged last tiles
    "bs37": dict(bs=37, knobs={}, counts=dict(_FUSED, gemm32_dw=0), group=_W3, colsum=0, plan=(PLAN_TILED, SCRATCH_ADD_C, COLSUM_NONE)),
    # 704 = 11 x 64 slots: fused SANB steps; gemm32_dw_kernel + ADD_C reducer: 7 x (dWu, dWd) + heads + fc
    "bs64": dict(bs=64, knobs={}, counts=dict(_FUSED, gemm32_dw=16), group=_W3, colsum=0, plan=(PLAN_DW, SCRATCH_ADD_C, COLSUM_NONE)),
    # the FOLDED column sums (rb.cs += in the reducer) exist only behind the separate launches, which 704 slots take when switched:
    # 7 merged weight-gradient launches + heads + fc on gemm32_dw_kernel, gate epilogue of the K = 64 kernel
    "bs64-separate": dict(bs=64, knobs=dict(sanb_fused=0), counts=dict(_SEPARATE, gemm32_dw=9), group=_W6, colsum=1,
                          plan=(PLAN_DW, SCRATCH_ADD_C, COLSUM_FOLDED)),
    # 4,224 = 66 x 64 slots >= SANB_FUSED_MAX_ROWS: the separate launches by default - n64f, k64 + gate epilogue, the merged
    # weight-gradient launch, the three fc layers as split-operand products (forward, dX, dW: 9) in three groups (the dW group accumulates)
    "bs384": dict(bs=384, knobs={}, counts=dict(_SEPARATE, gemm32_dw=8, gemm_x3=9, gemm_x3_group=3), group=_W6, colsum=1,
                  plan=(PLAN_DW, SCRATCH_ADD_C, COLSUM_FOLDED)),
    "bs384-two-dw-launches": dict(bs=384, knobs=dict(sidenet_dw_merge=0), counts=dict(_SEPARATE, gemm32_dw=15, gemm_x3=9, gemm_x3_group=3),
                                  group=_W3, colsum=1, plan=(PLAN_DW, SCRATCH_ADD_C, COLSUM_FOLDED)),
    # (no counter tells the gate epilogue from fuse_bwd_kernel: both follow a K = 64 launch.  The switch is the first condition of
    #  gemm32_k64_gate_ok, whose `false` sends bwd_step_separate to fuse_bwd_kernel.)
    "bs384-fuse-bwd-kernel": dict(bs=384, knobs=dict(gemm32_k64_gate=0), counts=dict(_SEPARATE, gemm32_dw=8, gemm_x3=9, gemm_x3_group=3),
                                  group=_W6, colsum=1, plan=(PLAN_DW, SCRATCH_ADD_C, COLSUM_FOLDED)),
}


@pytest.mark.parametrize("case", sorted(CACHED_CASES))
def test_cached_step_accumulates_into_nonzero_gradients_on_every_route(lib, case):
    """Header: "Gradients ... ACCUMULATING (+=) into them" (`iisan_side_net_bwd`, `iisan_sasrec_bwd`, `iisan_linear_bwd`).  The whole
    Cached step at the smallest sizes that reach each "+=" of the side network - see CACHED_CASES for which size and switch reaches which
    kernel; the route is asserted from the launch counters and, where the choice is made inside `launch_gemm32`, from `iisan_gemm32_plan`
    on the adapters' weight-gradient group of that size.  Two sizes do not reach a "+=" they are small enough to test by themselves and
    are run a second time with switches: the separate fusion kernels at 44 slots and the folded column sums at 704 slots exist only
    behind the separate SANB launches, which the product takes from 4,096 slots on (`sanb_fused` = 0 forces them below).
    Bounds: `test_cached_default_routes_match_the_cpu_oracle_at_bench_size` (GELU): 5e-4 of max|g|, 2e-3 for SASRec tensors and gates."""
    c = CACHED_CASES[case]
    ref, runs, counts, _ = _cached_two_backwards(c["bs"], c["knobs"])
    assert counts == c["counts"], (case, counts)
    M = c["bs"] * 11
    with _lib.dev(**c["knobs"]):
        pl = _plan(lib, c["group"](M), G32_DW, _side_scratch_floats(M, (768, 768, 768)), c["colsum"])
        # com_dense: iisan_linear_bwd has no executor scratch - always the tiled kernel's atomic "+=", colsum_kernel for the bias
        lin = _plan(lib, [(64, 192, M)], G32_DW, 0, 0)
    assert (pl[0], pl[3], pl[6]) == c["plan"], (case, pl)
    assert (lin[0], lin[3]) == (PLAN_TILED, SCRATCH_NONE), lin
    _accumulation_checks(runs, ref["G0"], ref["g"], _max_err, _route_tol, f"A cached {case}")


@pytest.mark.parametrize("sanb_fused", [1, 0])
def test_placeholder_gate_slots_leave_every_real_gradient_alone(lib, sanb_fused):
    """`fusion_method != "gated"`: the ABI's 21 gate slots are placeholders (`_SideNetBase._abi_params`), their gradient slots throw-away
    buffers (`ops._grad_targets`).  Every real parameter must still come out as G0 + g (125 tensors, same bounds and controls), the
    kernels must not write a gate gradient (`cfg.gated = 0`: the throw-away buffers stay zero) and the placeholders stay zero.  44
    slots, fused SANB steps and (switched) the separate launches."""
    seen = []
    real_targets = ops._grad_targets

    def spy(params):
        views, ret = real_targets(params)
        seen.extend(v for p, v in zip(params, views) if not p.requires_grad)
        return views, ret

    ops._grad_targets = spy
    try:
        ref, runs, counts, model = _cached_two_backwards(4, dict(sanb_fused=sanb_fused), fusion="sum")
    finally:
        ops._grad_targets = real_targets
    assert counts["sanb_fused_bwd"] == (7 if sanb_fused else 0), counts
    assert not any("side_gate" in k for k in ref["g"])
    _accumulation_checks(runs, ref["G0"], ref["g"], _max_err, _route_tol, f"A placeholders sanb_fused={sanb_fused}")
    assert len(seen) == 2 * 21, len(seen)                     # 21 gate slots per backward
    assert all(v.numel() == 1 and float(v.abs().max()) == 0.0 for v in seen)
    ph = model.mm_encoder._placeholders
    assert len(ph) == 21 and all(float(v.abs().max()) == 0.0 for v in ph.values())


def test_versa_step_accumulates_into_nonzero_gradients(lib):
    """Versa widths (1024 / 8192, bs = 128: 1,408 slots, as `test_alternative_routes_...`): the dim-align weight gradients - seven
    split-operand products with G32_HINT_B_EXACT16 in ONE accumulating group - and the widest reducer ([8192, 64] + column sums behind
    the merged weight-gradient launch).  Reference: the oracle's Versa side network + com_dense + SASRec + loss on the same taps."""
    n, bs = 500, 128
    b = synth.scientific_batch(bs=bs, seed=41, item_num=n, res=2, words=2)
    args = helpers.make_args(text_embedding_dim=8192, image_embedding_dim=1024, side_adapter_vit_list="3,7,11,15,19,23",
                             side_adapter_bert_list="4,19,34,49,64,79", image_layers=24, text_layers=80, drop_rate=0.0,
                             adapter_activation="GELU")
    model = helpers.build_model(args, n, b.pop_prob, cached="versa")
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters() if p.requires_grad}
    P = weights.fill_params_seeded(shapes, seed=555)
    helpers.load_trainables(model, P)
    g = torch.Generator().manual_seed(3)
    tabs = [torch.randn(n + 1, 7, d, generator=g) * 0.25 for d in (1024, 8192)]
    for t in tabs:
        t[0] = 0
    model.tap_stores = tuple(tapstore.TapStore(t.cuda(), range(7), "cuda", "fp32") for t in tabs)
    model.train()
    ids = b.ids.view(-1)
    Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    cv, text, mm = O.versa_side_network(tabs[0][ids], tabs[1][ids], Po, list(range(7)), list(range(7)), activation="GELU")
    score = torch.nn.functional.linear(torch.cat([cv, text, mm], 1), Po["com_dense.weight"], Po["com_dense.bias"])
    prec = O.sasrec(score.view(bs, 11, 64)[:, :-1], b.log_mask, Po, 2, 2).reshape(-1, 64)
    ref = O.inbatch_ce(b.ids, score, prec, b.log_mask, b.pop_prob)
    ref.backward()
    grads = {k: v.grad.detach() for k, v in Po.items()}
    G0 = _draw_g0(grads, seed=77)
    named = {k: p for k, p in model.named_parameters() if p.requires_grad}
    for k, p in named.items():
        p.grad = G0[k].cuda().clone()
    runs = []
    with _direct_param_grads():
        for _ in range(2):
            _zero_counts()
            loss = model(ids.cuda(), None, None, b.log_mask.cuda(), None)
            loss.backward()
            torch.cuda.synchronize()
            counts = _counts()
            assert abs(loss.item() - ref.item()) <= 3e-5 * abs(ref.item()), (loss.item(), ref.item())
            runs.append({k: p.grad.detach().cpu().clone() for k, p in named.items()})
    _zero_counts()
    # towers of different widths: no fused SANB step; 7 dim-align products forward + their 7 weight gradients on the split-operand route,
    # one group each; the merged weight-gradient launch of every step + the heads on gemm32_dw_kernel
    assert counts["sanb_fused_bwd"] == 0 and counts["gemm32_n64f"] == 7 and counts["gemm_x3"] == 14 and counts["gemm_x3_group"] == 2, counts
    M = bs * 11
    pl = _plan(lib, [(1024, 64, M), (8192, 64, M), (1024, 64, M), (64, 1024, M), (64, 8192, M), (64, 1024, M)], G32_DW,
               _side_scratch_floats(M, (1024, 8192, 1024)), 1)
    assert (pl[0], pl[3], pl[6]) == (PLAN_DW, SCRATCH_ADD_C, COLSUM_FOLDED), pl
    _accumulation_checks(runs, G0, grads, _max_err, _route_tol, "A versa bs128")


@functools.lru_cache(maxsize=None)
def _sasrec_reference(B, S, H, p):
    """Inputs, the generator's masks, the oracle's y / dx / parameter gradients for the loss (y * w).sum(), and G0."""
    E, L, seed = 64, 2, 987654321
    g = torch.Generator().manual_seed(B + S)
    pre = "user_encoder.transformer_encoder."
    P = {k[len(pre):]: v for k, v in weights.make_trainable_params(seed=99).items() if k.startswith(pre)}
    if S != 10:       # the position table of the fixture is [10, 64]: draw one of the right length
        P["position_embedding.weight"] = torch.randn(S, E, generator=g) * 0.1
    x = torch.randn(B, S, E, generator=g)
    lm = (torch.rand(B, S, generator=g) > 0.3).float()
    lm[:, -1] = 1
    w = torch.randn(B, S, E, generator=g)
    masks = None
    if p > 0:
        masks = {0: helpers.drop_factors(seed, 0, B * S * E, p).view(B, S, E)}
        for l in range(L):
            masks[1 + 3 * l] = helpers.drop_factors(seed, 1 + 3 * l, B * H * S * S, p).view(B, H, S, S)
            masks[2 + 3 * l] = helpers.drop_factors(seed, 2 + 3 * l, B * S * E, p).view(B, S, E)
            masks[3 + 3 * l] = helpers.drop_factors(seed, 3 + 3 * l, B * S * E, p).view(B, S, E)
    Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xo = x.clone().requires_grad_(True)
    yo = O.sasrec(xo, lm, Po, H, L, pre="", drop=masks)
    (yo * w).sum().backward()
    grads = {k: v.grad.detach() for k, v in Po.items()}
    return dict(P=P, x=x, lm=lm, w=w, y=yo.detach(), dx=xo.grad.detach(), g=grads, G0=_draw_g0(grads, seed=B * 100 + S),
                cfg=(S, E, H, L, p, seed), order=ops.sasrec_param_order(L))


@pytest.mark.parametrize("B,S,H,fused", [(130, 10, 2, 1), (130, 10, 2, 0), (33, 7, 4, 1), (33, 7, 4, 0), (20, 20, 2, 1)])
def test_sasrec_accumulates_into_nonzero_gradients(lib, B, S, H, fused):
    """`SasrecFn` alone on leaf tensors, dropout 0.1 with the generator's masks: the one-launch backward's fixed-order reducer
    (`sasrec_reduce_kernel`: G += sum of the workgroups' slabs) and, with `sasrec_fused` = 0, the per-operator launches (LayerNorm atomics,
    tiled atomic weight gradients, colsum_kernel).  S = 20 is outside the one-launch kernels: per-operator whatever the switch says.
    Norms and bounds of `test_sasrec_one_launch_kernels_...`: Frobenius, 2e-5 behind the one-launch backward, 1e-3 behind the other."""
    r = _sasrec_reference(B, S, H, 0.1)
    one_launch = bool(fused) and S <= 16
    tol = 2e-5 if one_launch else 1e-3
    cfg = ops.make_sasrec_cfg(*r["cfg"])
    params = [r["P"][k].cuda().requires_grad_(True) for k in r["order"]]
    for k, t in zip(r["order"], params):
        t.grad = r["G0"][k].cuda().clone()
    runs = []
    with _lib.dev(sasrec_fused=fused), _direct_param_grads():
        for _ in range(2):
            _zero_counts()
            xd = r["x"].cuda().requires_grad_(True)
            y = ops.SasrecFn.apply(cfg, xd, r["lm"].cuda(), *params)
            (y * r["w"].cuda()).sum().backward()
            torch.cuda.synchronize()
            assert _lib.dev_get("count:sasrec_fused_fwd") == (1 if one_launch else 0)
            assert _fro_err(y, r["y"], r["y"]) < 2e-5 and _fro_err(xd.grad, r["dx"], r["dx"]) < tol
            runs.append({k: t.grad.detach().cpu().clone() for k, t in zip(r["order"], params)})
    _zero_counts()
    _accumulation_checks(runs, r["G0"], r["g"], _fro_err, lambda k: tol, f"A sasrec B={B} S={S} H={H} fused={fused}")


@functools.lru_cache(maxsize=None)
def _side_problem(kind, M):
    """A side-network call on its own: cfg, parameter names in ABI order, parameters, taps, the weights w of the loss (item3 * w).sum()
    and the oracle's item3 / gradients.  kind "cached": 7 taps x 768; "versa": 7 + 7 taps x 1024 / 8192 with dim-align."""
    g = torch.Generator().manual_seed(M)
    if kind == "cached":
        names = ["mm_encoder." + k for k in ops.side_param_order(7, cached=True)]
        P = {k: v for k, v in weights.make_trainable_params(seed=556, cached=True).items() if k in names}
        dims = (768, 768)
        cfg = ops.make_side_cfg(7, 768, 64, 64, True, True, False, 7, 7, list(range(7)), 0)
    else:
        names = ["mm_encoder." + k for k in ops.versa_param_order(7, 7, True)]
        P = weights.fill_params_seeded({k: s for k, s in _versa_shapes().items() if k in names}, seed=555)
        dims = (1024, 8192)
        cfg = ops.make_versa_cfg(1024, 8192, 64, 64, True, True, False, 7, 7, list(range(7)), list(range(7)))
    assert set(names) == set(P)
    taps = [torch.randn(M, 7, d, generator=g) * 0.25 for d in dims]
    w = torch.randn(M, 192, generator=g)
    Po = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    if kind == "cached":
        out = O.side_network(taps[0], taps[1], Po, list(range(7)), activation="GELU", **CACHED_HEADS)
    else:
        out = O.versa_side_network(taps[0], taps[1], Po, list(range(7)), list(range(7)), activation="GELU")
    item3 = torch.cat(out, 1)
    (item3 * w).sum().backward()
    grads = {k: v.grad.detach() for k, v in Po.items()}
    return dict(cfg=cfg, names=names, P=P, taps=taps, w=w, item3=item3.detach(), g=grads, G0=_draw_g0(grads, seed=7 + M), dims=dims)


@functools.lru_cache(maxsize=None)
def _versa_shapes():
    """{state-dict key: shape} of the Versa configuration at BASELINE config 5 widths, from the product module itself."""
    args = helpers.make_args(text_embedding_dim=8192, image_embedding_dim=1024, side_adapter_vit_list="3,7,11,15,19,23",
                             side_adapter_bert_list="4,19,34,49,64,79", image_layers=24, text_layers=80, drop_rate=0.0,
                             adapter_activation="GELU")
    model = helpers.build_model(args, 50, torch.ones(51), cached="versa", device="cpu")
    return {k: tuple(p.shape) for k, p in model.named_parameters() if p.requires_grad}


def test_side_net_function_alone_accumulates_on_leaf_tensors(lib):
    """`SideNetFn` on leaf tensors (no model around it), 44 slots: the kernels receive the leaves' `.grad` themselves."""
    r = _side_problem("cached", 44)
    params = [r["P"][k].cuda().requires_grad_(True) for k in r["names"]]
    for k, t in zip(r["names"], params):
        t.grad = r["G0"][k].cuda().clone()
    tc, tt, w = r["taps"][0].cuda(), r["taps"][1].cuda(), r["w"].cuda()
    runs = []
    with _direct_param_grads():
        for _ in range(2):
            item3 = ops.SideNetFn.apply(r["cfg"], tc, tt, *params)
            (item3 * w).sum().backward()
            torch.cuda.synchronize()
            _close(item3, r["item3"], 2e-5, 2e-5, "item3")
            runs.append({k: t.grad.detach().cpu().clone() for k, t in zip(r["names"], params)})
    _zero_counts()
    _accumulation_checks(runs, r["G0"], r["g"], _max_err, _route_tol, "A SideNetFn alone, 44 slots")


def _linear_reference(M, K, N):
    g = torch.Generator().manual_seed(M + K + N)
    x, w, b, dy = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.1, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    ref = dict(y=x.double() @ w.double().t() + b.double(), dx=dy.double() @ w.double(), dw=dy.double().t() @ x.double(), db=dy.double().sum(0))
    G0 = _draw_g0(dict(dw=ref["dw"], db=ref["db"]), seed=M)
    return x, w, b, dy, ref, G0


def test_linear_function_alone_accumulates_on_leaf_tensors(lib):
    """`LinearFn` on leaf tensors against an fp64 `x @ w.T + b`: dw / db land in the leaves' non-zero `.grad`; two backwards."""
    x, w, b, dy, ref, G0 = _linear_reference(44, 192, 64)
    wd, bd = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    wd.grad, bd.grad = G0["dw"].cuda().clone(), G0["db"].cuda().clone()
    g = dict(dw=ref["dw"], db=ref["db"])
    runs = []
    with _direct_param_grads():
        for _ in range(2):
            xd = x.cuda().requires_grad_(True)
            y = ops.LinearFn.apply(xd, wd, bd)
            y.backward(dy.cuda())
            torch.cuda.synchronize()
            _close(y, ref["y"], 2e-5, 2e-5, "y")
            _close(xd.grad, ref["dx"], 2e-5, 2e-5, "dx")
            runs.append(dict(dw=wd.grad.detach().cpu().clone(), db=bd.grad.detach().cpu().clone()))
    _accumulation_checks(runs, G0, g, _max_err, lambda k: 5e-4, "A LinearFn alone")


# =====================================================================================================================================
# guard zones (B, C, D)
# =====================================================================================================================================

class Guarded:
    """`nbytes` of payload between two guard zones of GUARD bytes (a multiple of 4,096: the payload keeps its 16-byte alignment) filled
    with 0xA5, in ONE allocation: a write outside the payload lands in allocated memory and is seen by `intact()`."""

    def __init__(self, nbytes, dtype=torch.float32, shape=None, init=None):
        self.nbytes = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.nbytes,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.payload = self.buf[GUARD:GUARD + self.nbytes]
        self.t = self.payload.view(dtype) if self.nbytes % max(torch.empty((), dtype=dtype).element_size(), 1) == 0 else None
        if shape is not None:
            self.t = self.t.view(shape)
        if init is not None:
            self.t.copy_(init)
        self.ptr = self.buf.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    @classmethod
    def like(cls, t, init=None):
        t = torch.as_tensor(t)
        return cls(t.numel() * 4, torch.float32, tuple(t.shape), init)

    def intact(self):
        return bool((self.buf[:GUARD] == GUARD_BYTE).all()) and bool((self.buf[GUARD + self.nbytes:] == GUARD_BYTE).all())

    def bits(self):
        return self.payload.clone()


def _guards_intact(named):
    broken = [k for k, gd in named.items() if not gd.intact()]
    assert not broken, f"writes outside their own extent: {broken}"


# =====================================================================================================================================
# B. iisan_linear_fwd / iisan_linear_bwd, raw
# =====================================================================================================================================

@pytest.mark.parametrize("M,K,N", [(44, 192, 64), (407, 192, 64), (4224, 192, 64), (33, 72, 40), (1, 192, 64)])
def test_linear_entry_points_directly(lib, M, K, N):
    """`iisan_linear_fwd` / `iisan_linear_bwd` (com_dense; only ever seen through end-to-end losses): y and dx OVERWRITE a NaN prefill, dw
    and db accumulate into non-zero G0, each of dx / dw / db may be NULL - the other two are still right and the skipped tensor's buffer
    keeps its prefill bit for bit.  fp64 reference, the bound of `test_gemm32_vs_torch`'s accumulate case (2e-5, 2e-5); every output
    sits between guard zones."""
    x, w, b, dy, ref, G0 = _linear_reference(M, K, N)
    xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
    nan = float("nan")
    y = Guarded.like(ref["y"], init=torch.full((M, N), nan))
    _lib.check(lib.iisan_linear_fwd(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.ptr, M, K, N, _stream()), "iisan_linear_fwd")
    torch.cuda.synchronize()
    assert y.intact() and torch.isfinite(y.t).all()
    _close(y.t, ref["y"], 2e-5, 2e-5, "y")
    want = dict(dx=ref["dx"], dw=G0["dw"].double() + ref["dw"], db=G0["db"].double() + ref["db"])
    for skip in (None, "dx", "dw", "db"):
        out = dict(dx=Guarded.like(ref["dx"], init=torch.full((M, K), nan)), dw=Guarded.like(ref["dw"], init=G0["dw"]),
                   db=Guarded.like(ref["db"], init=G0["db"]))
        before = {k: v.bits() for k, v in out.items()}
        ptr = {k: (None if k == skip else v.ptr) for k, v in out.items()}
        _lib.check(lib.iisan_linear_bwd(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), ptr["dx"], ptr["dw"], ptr["db"], M, K, N, _stream()),
                   "iisan_linear_bwd")
        torch.cuda.synchronize()
        _guards_intact(out)
        for k, v in out.items():
            if k == skip:
                assert torch.equal(v.bits(), before[k]), f"{k} = NULL, yet its buffer changed"
                continue
            assert torch.isfinite(v.t).all(), k
            _close(v.t, want[k], 2e-5, 2e-5, f"{k} (skip {skip})")
        if skip is None:
            # negative control: the same comparison rejects what an overwriting and what a doubly adding kernel would leave
            for k in ("dw", "db"):
                assert _fails(_close, out[k].t, ref[k], 2e-5, 2e-5, k), f"{k}: the bound would accept an overwrite"
                assert _fails(_close, out[k].t, G0[k].double() + 2 * ref[k], 2e-5, 2e-5, k), f"{k}: the bound would accept a double add"


# =====================================================================================================================================
# C. d_loss on the four loss routes (+ D for the loss: guard zones)
# =====================================================================================================================================

CE_ROUTE_OF = {0: 0, 2: 1, 4: 2, 3: 3}       # ce_fast -> iisan_inbatch_ce_route: generic, row passes, fused f32 row pass, split operands
CE_SHAPES = [(37, 10), (3, 15), (7, 5), (64, 4)]
CE_CASES = [(f, bs, S) for f in (0, 2, 4, 3) for bs, S in CE_SHAPES] + [(0, 5, 10)]


@functools.lru_cache(maxsize=None)
def _ce_problem(bs, S):
    """Ragged sequence lengths, history padding, a duplicated item (the false-negative mask) - the recipe of
    `test_split_operand_ce_matches_the_oracle_on_ragged_shapes` - and the fp64 loss / gradients of `O.inbatch_ce`."""
    seed = bs + S
    rnd = random.Random(seed)
    lengths = [rnd.randint(2, S + 1) for _ in range(bs)]
    n = max(40, bs * 3)
    b = synth.scientific_batch(bs=bs, seed=90 + seed, item_num=n, res=2, words=2, lengths=lengths, dup_items=True, seq_len=S)
    g = torch.Generator().manual_seed(seed)
    score = torch.randn(bs * (S + 1), 64, generator=g) * 0.4
    prec = torch.randn(bs * S, 64, generator=g) * 0.4
    so, po = score.double().requires_grad_(True), prec.double().requires_grad_(True)
    ref = O.inbatch_ce(b.ids, so, po, b.log_mask.double(), b.pop_prob.double())
    ref.backward()
    return b, score, prec, ref.item(), so.grad.detach(), po.grad.detach()


class CeCall:
    """One loss problem on the device with its workspace and outputs between guard zones, `ws_bytes` = the query's answer exactly."""

    def __init__(self, lib, bs, S):
        b, score, prec, *_ = _ce_problem(bs, S)
        self.lib, self.bs, self.S = lib, bs, S
        self.ids, self.lm, self.pop = b.ids.view(-1).cuda(), b.log_mask.cuda(), b.pop_prob.cuda()
        self.score, self.prec = score.cuda(), prec.cuda()
        self.need = lib.iisan_inbatch_ce_ws_bytes(bs, S)
        assert self.need > 0 and self.need % 16 == 0
        self.ws = Guarded(self.need, torch.uint8)
        self.loss = Guarded(4, init=torch.tensor([float("nan")]))
        self.d_score, self.d_prec = Guarded.like(score), Guarded.like(prec)
        self.tok = C.c_uint64(0)

    def fwd(self, ws_ptr="own", ws_bytes=None):
        return self.lib.iisan_inbatch_ce_fwd(self.ids.data_ptr(), self.score.data_ptr(), self.prec.data_ptr(), self.lm.data_ptr(),
                                             self.pop.data_ptr(), self.pop.numel(), self.bs, self.S, 64, self.loss.ptr,
                                             self.ws.ptr if ws_ptr == "own" else ws_ptr, self.need if ws_bytes is None else ws_bytes,
                                             C.byref(self.tok), _stream())

    def bwd(self, d_loss, token=None, ws_ptr="own", ws_bytes=None):
        return self.lib.iisan_inbatch_ce_bwd(self.ids.data_ptr(), self.score.data_ptr(), self.prec.data_ptr(), self.lm.data_ptr(),
                                             self.pop.data_ptr(), self.bs, self.S, 64, d_loss, self.d_score.ptr, self.d_prec.ptr,
                                             self.ws.ptr if ws_ptr == "own" else ws_ptr, self.need if ws_bytes is None else ws_bytes,
                                             self.tok.value if token is None else token, _stream())

    def nan_outputs(self):
        self.d_score.t.fill_(float("nan"))
        self.d_prec.t.fill_(float("nan"))

    def guards(self):
        return dict(ws=self.ws, loss=self.loss, d_score=self.d_score, d_prec=self.d_prec)


@pytest.mark.parametrize("ce_fast,bs,S", CE_CASES)
def test_d_loss_is_a_plain_multiplier_on_every_loss_route(lib, ce_fast, bs, S):
    """`iisan_inbatch_ce_bwd`: "d_loss: host scalar multiplier ... d_score and d_prec are overwritten".  One forward, then the backward
    five times on the same workspace and token with d_loss = 1, 0.5, -2, -0.3, 1, d_score / d_prec prefilled with NaN each time:
      * 0.5 and -2: BIT-equal to that factor times the d_loss = 1 result (no atomics in this backward; a power of two scales
        d_loss / nvalid, every product and every sum exactly) - a factor that enters twice, not at all or not linearly differs;
      * the last call BIT-equal to the first: the backward does not modify what the forward left in the workspace (the fused and the
        split-operand routes keep d_prec for d_loss = 1 there and only scale it);
      * -0.3: against -0.3 x the fp64 gradient of `O.inbatch_ce`, the bound of the ragged-shape loss test (2e-4 of the scale + 1e-9).
    Shapes: ragged 16-row tiles, RS1 = 16 (S = 15), S = 5, S = 4 (the plain kernel under every switch), and for the generic route
    S = 10 once more at a batch of 5 (T = 50, M = 55: the plain kernel's column pass over four X blocks, the last one partial).  Workspace
    of exactly `iisan_inbatch_ce_ws_bytes`, guard zones around it, the loss and both gradients."""
    b, _, _, loss_ref, ds_ref, dp_ref = _ce_problem(bs, S)
    want_route = 0 if (ce_fast == 0 or S < 5) else CE_ROUTE_OF[ce_fast]
    res = {}
    with _lib.dev(ce_fast=ce_fast):
        assert lib.iisan_inbatch_ce_route(bs, S) == want_route
        c = CeCall(lib, bs, S)
        _lib.check(c.fwd(), "iisan_inbatch_ce_fwd")
        for i, d in enumerate((1.0, 0.5, -2.0, -0.3, 1.0)):
            c.nan_outputs()
            _lib.check(c.bwd(d), "iisan_inbatch_ce_bwd")
            torch.cuda.synchronize()
            res[i] = (c.d_score.t.cpu().clone(), c.d_prec.t.cpu().clone())
    _lib.dev_set("count:ce16", 0)
    _guards_intact(c.guards())
    loss = c.loss.t.item()
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref), (loss, loss_ref)
    for i in res:
        assert torch.isfinite(res[i][0]).all() and torch.isfinite(res[i][1]).all(), i
    for i, f in ((1, 0.5), (2, -2.0)):
        for got, one, what in zip(res[i], res[0], ("d_score", "d_prec")):
            assert torch.equal(got, one * f), (what, f, (got - one * f).abs().max().item())
    for got, one, what in zip(res[4], res[0], ("d_score", "d_prec")):
        assert torch.equal(got, one), f"{what}: the backward changed what a later backward on the same workspace computes"
    _close(res[3][0], -0.3 * ds_ref, 2e-4, 1e-9, "d_score at d_loss = -0.3")
    _close(res[3][1], -0.3 * dp_ref, 2e-4, 1e-9, "d_prec at d_loss = -0.3")
    # (the bound means something: it rejects d_loss ignored and d_loss applied twice)
    assert _fails(_close, res[3][0], ds_ref, 2e-4, 1e-9, "") and _fails(_close, res[3][0], 0.09 * ds_ref, 2e-4, 1e-9, "")
    e = max(_max_err(res[3][0], -0.3 * ds_ref, ds_ref), _max_err(res[3][1], -0.3 * dp_ref, dp_ref)) / 0.3
    print(f"abi-contracts C ce_fast={ce_fast} route={want_route} bs={bs} S={S}: worst err / scale at d_loss=-0.3 {e:.2e} (bound 2e-4)")


@pytest.mark.parametrize("ce_fast", [0, 2, 4, 3])
def test_loss_with_a_workspace_one_byte_short_launches_nothing(lib, ce_fast):
    """`need - 1` bytes, and a NULL workspace: IISAN_EWORKSPACE from the forward and from the backward, `iisan_last_error` names the
    workspace, and after a synchronise the loss / d_score / d_prec still hold their prefill: nothing was launched.  The backward
    with `fwd_token = 0` is IISAN_EBADSHAPE and leaves the outputs alone as well."""
    bs, S = 37, 10
    with _lib.dev(ce_fast=ce_fast):
        c = CeCall(lib, bs, S)
        c.nan_outputs()
        before = {k: v.bits() for k, v in c.guards().items()}
        for ws_ptr, nbytes in (("own", c.need - 1), (None, c.need)):
            assert c.fwd(ws_ptr, nbytes) == IISAN_EWORKSPACE
            assert b"workspace" in lib.iisan_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(v.bits(), before[k]) for k, v in c.guards().items())
        _lib.check(c.fwd(), "iisan_inbatch_ce_fwd")
        torch.cuda.synchronize()
        before = {k: v.bits() for k, v in c.guards().items()}
        for ws_ptr, nbytes in (("own", c.need - 1), (None, c.need)):
            assert c.bwd(1.0, None, ws_ptr, nbytes) == IISAN_EWORKSPACE
            assert b"workspace" in lib.iisan_last_error()
        assert c.bwd(1.0, token=0) == IISAN_EBADSHAPE
        torch.cuda.synchronize()
        assert all(torch.equal(v.bits(), before[k]) for k, v in c.guards().items())
    _lib.dev_set("count:ce16", 0)


# =====================================================================================================================================
# D. workspace of the side network and of SASRec: sufficient, respected, necessary
# =====================================================================================================================================

class SideCall:
    """One raw `iisan_side_net_fwd` / `_bwd` problem: workspace of exactly `iisan_side_net_ws_bytes`, item3 and every gradient tensor
    (prefilled with G0) between guard zones of their own."""

    def __init__(self, lib, kind, M):
        r = self.r = _side_problem(kind, M)
        self.lib, self.M, self.cfg = lib, M, r["cfg"]
        assert lib.iisan_side_net_num_params(C.byref(self.cfg)) == len(r["names"])
        self.params = [r["P"][k].cuda().contiguous() for k in r["names"]]
        self.ptab = ops._ptr_table(self.params)
        self.taps = [t.cuda().contiguous() for t in r["taps"]]
        self.w = r["w"].cuda().contiguous()
        self.need = lib.iisan_side_net_ws_bytes(C.byref(self.cfg), M)
        assert self.need > 0
        self.ws = Guarded(self.need, torch.uint8)
        self.item3 = Guarded.like(r["item3"], init=torch.full((M, 192), float("nan")))
        self.grads = {k: Guarded.like(r["G0"][k], init=r["G0"][k]) for k in r["names"]}
        self.gtab = (C.c_void_p * len(r["names"]))(*[self.grads[k].ptr for k in r["names"]])
        self.tok = C.c_uint64(0)

    def fwd(self, ws_ptr="own", ws_bytes=None):
        return self.lib.iisan_side_net_fwd(C.byref(self.cfg), self.taps[0].data_ptr(), self.taps[1].data_ptr(), self.M, self.ptab, self.item3.ptr,
                                           self.ws.ptr if ws_ptr == "own" else ws_ptr, self.need if ws_bytes is None else ws_bytes,
                                           C.byref(self.tok), _stream())

    def bwd(self, token=None, ws_ptr="own", ws_bytes=None):
        return self.lib.iisan_side_net_bwd(C.byref(self.cfg), self.taps[0].data_ptr(), self.taps[1].data_ptr(), self.M, self.ptab, self.w.data_ptr(),
                                           self.gtab, self.ws.ptr if ws_ptr == "own" else ws_ptr, self.need if ws_bytes is None else ws_bytes,
                                           self.tok.value if token is None else token, _stream())

    def guards(self):
        return dict(self.grads, ws=self.ws, item3=self.item3)


@pytest.mark.parametrize("kind,M,knobs", [("cached", 44, {}), ("cached", 407, {}), ("cached", 407, dict(sanb_fused=0)),
                                          ("versa", 44, {}), ("versa", 407, {}), ("versa", 407, dict(x3=2))])
def test_side_net_stays_inside_its_workspace_and_its_outputs(lib, kind, M, knobs):
    """`iisan_side_net_ws_bytes` is sufficient and respected at ragged sizes (44 and 407 item slots; Cached 768 / 768 on the fused and on
    the separate SANB launches, Versa 1024 / 8192 with dim-align, also with every eligible product on the split-operand route, whose
    operand images are the largest carve of the workspace): `ws_bytes` = the query's answer exactly, guard zones around the workspace,
    item3 and each of the gradient tensors.  After forward + backward every guard byte is unchanged, item3 matches the oracle (2e-5)
    and the gradients are G0 + g within the route bounds (5e-4, gates 2e-3) - the raw `+=` of `iisan_side_net_bwd`, with its controls."""
    with _lib.dev(**knobs):
        c = SideCall(lib, kind, M)
        _lib.check(c.fwd(), "iisan_side_net_fwd")
        _lib.check(c.bwd(), "iisan_side_net_bwd")
        torch.cuda.synchronize()
    _zero_counts()
    _guards_intact(c.guards())
    r = c.r
    _close(c.item3.t, r["item3"], 2e-5, 2e-5, "item3")
    got = {k: v.t.cpu().clone() for k, v in c.grads.items()}
    w = _assert_accumulated(got, r["G0"], r["g"], 1, _max_err, _route_tol, f"D side net {kind} M={M}")
    _assert_rejected(got, r["G0"], r["g"], 0, 1, _max_err, _route_tol, "against g alone (an overwrite)")
    _assert_rejected(got, r["G0"], r["g"], 1, 2, _max_err, _route_tol, "against G0 + 2 g (a double add)")
    print(f"abi-contracts D side net {kind} M={M} {knobs}: ws {c.need} bytes, worst err/bound {w[0]:.3f} ({w[1]} {w[2]:.2e})")


@pytest.mark.parametrize("kind", ["cached", "versa"])
def test_side_net_with_a_workspace_one_byte_short_launches_nothing(lib, kind):
    """`need - 1` bytes and a NULL workspace: IISAN_EWORKSPACE, the message names the workspace, item3 / the gradients keep their prefill
    after a synchronise.  `iisan_side_net_bwd` with `fwd_token = 0`: IISAN_EBADSHAPE, gradients untouched."""
    c = SideCall(lib, kind, 44)
    before = {k: v.bits() for k, v in c.guards().items()}
    for ws_ptr, nbytes in (("own", c.need - 1), (None, c.need)):
        assert c.fwd(ws_ptr, nbytes) == IISAN_EWORKSPACE
        assert b"workspace" in lib.iisan_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(v.bits(), before[k]) for k, v in c.guards().items())
    _lib.check(c.fwd(), "iisan_side_net_fwd")
    torch.cuda.synchronize()
    before = {k: v.bits() for k, v in c.guards().items()}
    for ws_ptr, nbytes in (("own", c.need - 1), (None, c.need)):
        assert c.bwd(None, ws_ptr, nbytes) == IISAN_EWORKSPACE
        assert b"workspace" in lib.iisan_last_error()
    assert c.bwd(token=0) == IISAN_EBADSHAPE
    assert b"fwd_token" in lib.iisan_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(v.bits(), before[k]) for k, v in c.guards().items())
    _zero_counts()


class SasrecCall:
    """One raw `iisan_sasrec_fwd` / `_bwd` problem between guard zones (workspace, y, dx, every gradient tensor prefilled with G0)."""

    def __init__(self, lib, B, S, H):
        r = self.r = _sasrec_reference(B, S, H, 0.1)
        self.lib, self.B = lib, B
        self.cfg = ops.make_sasrec_cfg(*r["cfg"])
        self.params = [r["P"][k].cuda().contiguous() for k in r["order"]]
        self.ptab = ops._ptr_table(self.params)
        self.x, self.lm, self.dy = r["x"].cuda(), r["lm"].cuda(), r["w"].cuda()
        self.need = lib.iisan_sasrec_ws_bytes(C.byref(self.cfg), B)
        assert self.need > 0
        self.ws = Guarded(self.need, torch.uint8)
        nan = torch.full(tuple(r["x"].shape), float("nan"))
        self.y, self.dx = Guarded.like(r["x"], init=nan), Guarded.like(r["x"], init=nan)
        self.grads = {k: Guarded.like(r["G0"][k], init=r["G0"][k]) for k in r["order"]}
        self.gtab = (C.c_void_p * len(r["order"]))(*[self.grads[k].ptr for k in r["order"]])

    def fwd(self, ws_ptr="own", ws_bytes=None):
        return self.lib.iisan_sasrec_fwd(C.byref(self.cfg), self.x.data_ptr(), self.lm.data_ptr(), self.B, self.ptab, self.y.ptr,
                                         self.ws.ptr if ws_ptr == "own" else ws_ptr, self.need if ws_bytes is None else ws_bytes, _stream())

    def bwd(self, ws_ptr="own", ws_bytes=None):
        return self.lib.iisan_sasrec_bwd(C.byref(self.cfg), self.x.data_ptr(), self.lm.data_ptr(), self.B, self.ptab, self.dy.data_ptr(),
                                         self.dx.ptr, self.gtab, self.ws.ptr if ws_ptr == "own" else ws_ptr,
                                         self.need if ws_bytes is None else ws_bytes, _stream())

    def guards(self):
        return dict(self.grads, ws=self.ws, y=self.y, dx=self.dx)


@pytest.mark.parametrize("B,S,H,fused", [(33, 7, 4, 1), (33, 7, 4, 0), (130, 10, 2, 1), (130, 10, 2, 0)])
def test_sasrec_stays_inside_its_workspace_and_its_outputs(lib, B, S, H, fused):
    """`iisan_sasrec_ws_bytes` is sufficient and respected by the one-launch kernels (ragged last workgroup: 33 = 5 x 6 + 3 sequences at
    S = 7, 130 = 32 x 4 + 2 at S = 10; the slab of per-workgroup partial sums is the last carve) and by the per-operator launches.  y and
    dx overwrite a NaN prefill, the gradients are G0 + g; bounds of the one-launch test (2e-5 / 1e-3, Frobenius), with the controls."""
    tol = 2e-5 if fused else 1e-3
    with _lib.dev(sasrec_fused=fused):
        c = SasrecCall(lib, B, S, H)
        _lib.check(c.fwd(), "iisan_sasrec_fwd")
        _lib.check(c.bwd(), "iisan_sasrec_bwd")
        torch.cuda.synchronize()
    _zero_counts()
    _guards_intact(c.guards())
    r = c.r
    assert torch.isfinite(c.y.t).all() and torch.isfinite(c.dx.t).all()
    assert _fro_err(c.y.t, r["y"], r["y"]) < 2e-5 and _fro_err(c.dx.t, r["dx"], r["dx"]) < tol
    got = {k: v.t.cpu().clone() for k, v in c.grads.items()}
    w = _assert_accumulated(got, r["G0"], r["g"], 1, _fro_err, lambda k: tol, f"D sasrec B={B} fused={fused}")
    _assert_rejected(got, r["G0"], r["g"], 0, 1, _fro_err, lambda k: tol, "against g alone (an overwrite)")
    _assert_rejected(got, r["G0"], r["g"], 1, 2, _fro_err, lambda k: tol, "against G0 + 2 g (a double add)")
    print(f"abi-contracts D sasrec B={B} S={S} H={H} fused={fused}: ws {c.need} bytes, worst err/bound {w[0]:.3f} ({w[1]} {w[2]:.2e})")


@pytest.mark.parametrize("fused", [1, 0])
def test_sasrec_with_a_workspace_one_byte_short_launches_nothing(lib, fused):
    """`need - 1` bytes and a NULL workspace: IISAN_EWORKSPACE from both directions, the message names the workspace, nothing launched."""
    with _lib.dev(sasrec_fused=fused):
        c = SasrecCall(lib, 33, 7, 4)
        before = {k: v.bits() for k, v in c.guards().items()}
        for ws_ptr, nbytes in (("own", c.need - 1), (None, c.need)):
            assert c.fwd(ws_ptr, nbytes) == IISAN_EWORKSPACE
            assert b"workspace" in lib.iisan_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(v.bits(), before[k]) for k, v in c.guards().items())
        _lib.check(c.fwd(), "iisan_sasrec_fwd")
        torch.cuda.synchronize()
        before = {k: v.bits() for k, v in c.guards().items()}
        for ws_ptr, nbytes in (("own", c.need - 1), (None, c.need)):
            assert c.bwd(ws_ptr, nbytes) == IISAN_EWORKSPACE
            assert b"workspace" in lib.iisan_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(v.bits(), before[k]) for k, v in c.guards().items())
    _zero_counts()
