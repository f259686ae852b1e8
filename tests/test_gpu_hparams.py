"""The trainable path at launcher arguments OTHER than the reference launcher's defaults (bottleneck 64, `max_seq_len` 10, 2 heads,
2 blocks, seven SANBs): every other GPU test of the side network, SASRec, the loss and the eval path runs at those defaults, the
library accepts far more.

  a. a Cached training step against `O.model_loss_from_taps` in float64 - bottleneck widths 4 / 16 / 32 / 128 (the whole SANB chain on
     the generic tiled products: `sanb_fused_ok`, the n64f kernel and the K = 64 kernel with its gate epilogue all need 64), "sum" fusion,
     one and thirteen SANBs, windows of 5 .. 32 positions with 1 .. 4 heads and 1 .. 8 blocks (from S = 16 on the loss takes its generic
     route, from S = 17 on SASRec its per-operator launches), a batch whose loss is exactly zero;
  b. `ops.SasrecFn` alone against `O.sasrec` in float64 at d_model 128 / 256 (reachable through the ABI only) and S = 1 / 32;
  c. the loss alone against `O.inbatch_ce` in float64 from S = 1 to S = 63, S = 0 and S = 64 refused;
  d. eval at windows of 20 and 5 positions on histories longer than the window (`evaluate._pack_users` truncates them).

`tests/test_oracle_vs_golden.py::test_sidenet_at_non_default_hyperparameters_matches_reference` pins the oracle to the real reference at
these settings.  Bounds are the ones `test_gpu_trainable.py` / `test_gpu_abi_contracts.py` hold the same tensors to; every reference
carries its own conditioning check (the float32 oracle against the float64 one, a quarter of the bound at most: what is left of the
bound is the kernels') and every comparison its negative control.  Measured errors: `profiles/hparams_parity.md`."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import _lib, evaluate, ops, synth, tapstore, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

IISAN_EBADSHAPE = -1
CACHED_HEADS = dict(cv_head="mm_encoder.cv_pre_fc.", text_head="mm_encoder.bert_pre_fc.")
COUNTERS = ("sanb_fused_fwd", "sanb_fused_bwd", "gemm32_n64f", "gemm32_k64", "gemm32_dw", "gemm_x3", "gemm_x3_group", "sasrec_fused_fwd", "ce16")
N_ITEMS = 500
ALL_LAYERS = ",".join(str(i) for i in range(12))
ONE_SANB_BIAS = "mm_encoder.mm_adapter_list.0.fc_up.bias"       # the tensor the negative controls zero


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _counts():
    return {n: _lib.dev_get("count:" + n) for n in COUNTERS}


def _zero_counts():
    for n in COUNTERS:
        _lib.dev_set("count:" + n, 0)


def _max_err(got, want):
    """max|got - want| / max|want|: the per-tensor figure of the GELU route tests."""
    return ((_f64(got) - _f64(want)).abs().max() / (_f64(want).abs().max() + 1e-300)).item()


def _fro_err(got, want):
    """|got - want| / |want| in the Frobenius norm: the figure of the ReLU route test and of the SASRec tests."""
    return ((_f64(got) - _f64(want)).norm() / (_f64(want).norm() + 1e-300)).item()


# =====================================================================================================================================
# a. Cached training step
# =====================================================================================================================================

def _case(down=64, act="RELU", fusion="gated", lists="1,3,5,7,9,11", rmfirst=False, S=10, H=2, L=2):
    return dict(cv_adapter_down_size=down, bert_adapter_down_size=down, adapter_activation=act, fusion_method=fusion,
                side_adapter_vit_list=lists, side_adapter_bert_list=lists, remove_first="TRUE" if rmfirst else "None",
                max_seq_len=S, num_attention_heads=H, transformer_block=L)


STEP_CASES = {f"down{r}_{act.lower()}": _case(down=r, act=act) for r in (4, 16, 32, 128) for act in ("RELU", "GELU")}
STEP_CASES.update({
    "down32_sum": _case(down=32, fusion="sum"),
    "one_sanb_rmfirst": _case(lists="11", rmfirst=True),
    "thirteen_sanbs": _case(lists=ALL_LAYERS),
    "s5_h1_l1": _case(S=5, H=1, L=1),
    "s15_h4_l2": _case(S=15, H=4, L=2),
    "s16_h4_l2": _case(S=16, H=4, L=2),          # seq x heads = 64
    "s16_h2_l3": _case(S=16, H=2, L=3),
    "s17_h2_l2": _case(S=17, H=2, L=2),          # the first window outside the one-launch SASRec kernels
    "s20_h2_l3": _case(S=20, H=2, L=3),
    "s32_h2_l1": _case(S=32, H=2, L=1),
    "s32_h1_l8": _case(S=32, H=1, L=8),
    "down32_s20_h4_l3_gelu": _case(down=32, act="GELU", S=20, H=4, L=3),
})
# Batch seed per (case, batch size): 45 unless that batch's reference is ill-conditioned (`_step_problem` asserts it; the first seed
# from 45 on whose float32 oracle stays within a quarter of every bound of the float64 one - a property of the reference alone).
STEP_SEEDS = {("s32_h1_l8", 37): 47}          # (45: float32 oracle 1.6e-3 off the float64 one on block 0's w_Q - 32 x the bound; 46: 10 x)


def _lengths(bs, S, seed):
    """Ragged lengths (target included): one sequence of full length S + 1, one of length 2, the rest uniform between."""
    rnd = random.Random(seed)
    return ([S + 1, 2] + [rnd.randint(2, S + 1) for _ in range(bs - 2)])[:bs] if bs > 1 else [7]


@functools.lru_cache(maxsize=None)
def _tap_tables():
    """[N_ITEMS + 1, 13, 768] per modality (every hidden state: each case's store packs the layers its side network reads); row 0 = the
    padding item."""
    g = torch.Generator().manual_seed(5)
    tabs = [torch.randn(N_ITEMS + 1, 13, 768, generator=g) * 0.25 for _ in range(2)]
    for t in tabs:
        t[0] = 0
    return tabs


def _step_errors(got, want, act):
    """{tensor (or, ReLU: a tower's gate vector): (error, bound)} in the norms and bounds of
    `test_gpu_trainable.py::test_cached_default_routes_match_the_cpu_oracle_at_bench_size`: GELU adapters max-abs over the tensor's
    scale, 5e-4 (SASRec tensors and the one-scalar gates 2e-3); ReLU adapters (a flipped unit moves single elements) relative Frobenius,
    5e-5, a tower's gates held together as the vector they form."""
    out, gates = {}, {}
    assert set(got) == set(want)
    for k in want:
        if act == "GELU":
            out[k] = (_max_err(got[k], want[k]), 2e-3 if ("user_encoder" in k or "side_gate" in k) else 5e-4)
        elif "side_gate" in k:
            gates.setdefault(k.rsplit(".", 1)[0], []).append((_f64(got[k]).reshape(-1), _f64(want[k]).reshape(-1)))
        else:
            out[k] = (_fro_err(got[k], want[k]), 5e-5)
    for tower, pairs in gates.items():
        out[tower] = (_fro_err(torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs])), 5e-5)
    return out


def _check_step(loss, grads, prob):
    """Loss within 2e-5 relative, every gradient within its bound.  Returns {family: worst error / bound} for the report."""
    assert np.isfinite(loss) and abs(loss - prob["loss"]) <= 2e-5 * abs(prob["loss"]), (loss, prob["loss"])
    errs = _step_errors(grads, prob["g"], prob["act"])
    bad = sorted(((e / tol, k, e) for k, (e, tol) in errs.items() if not e < tol), reverse=True)
    assert not bad, f"{len(bad)} tensors off the float64 oracle: {bad[:4]}"
    return errs


@functools.lru_cache(maxsize=None)
def _step_problem(case, bs):
    """Batch, parameters (shapes from the product's module tree), the float64 oracle's loss and gradients - computed once per
    (case, batch size), shared by the route knobs, never modified - and the conditioning check of the reference itself."""
    kw = STEP_CASES[case]
    S, act = kw["max_seq_len"], kw["adapter_activation"]
    seed = STEP_SEEDS.get((case, bs), 45)
    b = synth.scientific_batch(bs=bs, seed=seed, seq_len=S, item_num=N_ITEMS, res=2, words=2, lengths=_lengths(bs, S, seed), dup_items=True)
    if bs > 1:
        real = (b.ids != 0).sum(1)
        assert int(real.max()) == S + 1 and int(real.min()) == 2
    args = helpers.make_args(drop_rate=0.0, **kw)
    shapes = {k: tuple(p.shape) for k, p in helpers.build_model(args, N_ITEMS, b.pop_prob, cached=True, device="cpu").named_parameters()
              if p.requires_grad}
    P = weights.fill_params_seeded(shapes, seed=557)
    rm = kw["remove_first"] == "TRUE"
    layers = O.side_layer_list(kw["side_adapter_vit_list"], rm)
    tabs = _tap_tables()
    ids = b.ids.view(-1)
    out = {}
    for dt in (torch.float32, torch.float64):
        Po = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in P.items()}
        loss, _ = O.model_loss_from_taps(ids, tabs[0][ids].to(dt), tabs[1][ids].to(dt), b.log_mask.to(dt), b.pop_prob.to(dt), Po, layers,
                                         heads=kw["num_attention_heads"], n_layers=kw["transformer_block"], activation=act,
                                         fusion=kw["fusion_method"], remove_first=rm, **CACHED_HEADS)
        loss.backward()
        out[dt] = (loss.item(), {k: v.grad.detach() for k, v in Po.items()})
    loss, grads = out[torch.float64]
    prob = dict(case=case, bs=bs, kw=kw, act=act, b=b, P=P, loss=loss, g=grads, floor={})
    if bs > 1:
        prob["floor"] = _step_errors(out[torch.float32][1], grads, act)
        worst = max((e / tol, k, e) for k, (e, tol) in prob["floor"].items())
        assert worst[0] <= 0.25, f"an ill-conditioned reference (float32 oracle vs float64 oracle, error / bound {worst}): choose another batch"
    return prob


def _gpu_step(prob, knobs):
    b = prob["b"]
    args = helpers.make_args(drop_rate=0.0, **prob["kw"])
    model = helpers.build_model(args, N_ITEMS, b.pop_prob, cached=True)
    helpers.load_trainables(model, prob["P"])
    layers = model.mm_encoder.packed_layers()
    model.tap_stores = tuple(tapstore.TapStore(t, layers, "cuda", "fp32") for t in _tap_tables())
    model.train()
    with _lib.dev(**knobs):
        _zero_counts()
        loss = model(b.ids.view(-1).cuda(), None, None, b.log_mask.cuda(), None)
        loss.backward()
        torch.cuda.synchronize()
        counts = _counts()
    _zero_counts()
    grads = {}
    for k, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None, k
            grads[k] = p.grad.detach().cpu()
    return loss.item(), grads, counts, model


def _report(tag, errs):
    fam = {}
    for k, (e, tol) in errs.items():
        f = ("gate" if "side_gate" in k else "sasrec" if "user_encoder" in k else "adapter" if "adapter_list" in k else "fc/head")
        fam[f] = max(fam.get(f, (0.0, tol)), (e, tol))
    print(f"hparams {tag}: " + ", ".join(f"{f} {e:.2e} (bound {tol:.0e})" for f, (e, tol) in sorted(fam.items())))


@pytest.mark.parametrize("bs", [3, 37])
@pytest.mark.parametrize("case", list(STEP_CASES))
def test_cached_step_at_non_default_hyperparameters_matches_the_fp64_oracle(lib, case, bs):
    """One Cached training step (tap stores, default knobs; where the bottleneck is 64 also `sanb_fused` 0 and 2) at 33 .. 99 and at
    407 .. 1,221 item slots (ragged, >= 256 rows: the K threshold of the weight-gradient products' split) against the float64 oracle on the
    same taps and parameters.  With a bottleneck other than 64 the launch counters must show the generic chain: no fused SANB launch, no
    n64f launch, and of the K = 64 kernel only the one product that has nothing to do with the bottleneck (dY = dE Wh of the three heads:
    K = embedding_dim = 64, N = 768)."""
    prob = _step_problem(case, bs)
    kw = prob["kw"]
    down, S = kw["cv_adapter_down_size"], kw["max_seq_len"]
    # negative control: the same assertion rejects the oracle's own result with one SANB's fc_up.bias gradient zeroed
    _check_step(prob["loss"], prob["g"], prob)
    broken = dict(prob["g"])
    broken[ONE_SANB_BIAS] = torch.zeros_like(broken[ONE_SANB_BIAS])
    assert _fails(_check_step, prob["loss"], broken, prob)
    assert _fails(_check_step, prob["loss"] * (1 + 1e-4), prob["g"], prob)
    for knob in ((1, 0, 2) if down == 64 else (1,)):
        loss, grads, c, _ = _gpu_step(prob, {} if knob == 1 else dict(sanb_fused=knob))
        errs = _check_step(loss, grads, prob)
        _report(f"{case} bs={bs} sanb_fused={knob} loss {abs(loss - prob['loss']) / abs(prob['loss']):.1e}", errs)
        if down != 64:
            assert c["sanb_fused_fwd"] == 0 and c["sanb_fused_bwd"] == 0 and c["gemm32_n64f"] == 0 and c["gemm32_k64"] == 1, c
        elif knob == 0:
            assert c["sanb_fused_fwd"] == 0 and c["sanb_fused_bwd"] == 0 and c["gemm32_n64f"] > 0, c
        else:
            assert c["sanb_fused_fwd"] > 0 and c["sanb_fused_bwd"] > 0 and c["gemm32_n64f"] == 0, c
        assert c["sasrec_fused_fwd"] == (1 if S <= 16 else 0), c
        assert c["ce16"] == 0, c
    assert lib.iisan_inbatch_ce_route(bs, S) == (0 if (S < 5 or S >= 16) else 2)


def test_a_batch_of_one_sequence_has_zero_loss_and_zero_gradients(lib):
    """bs = 1, one sequence of 7 items: every other column of a row's logits is either padding or an item of the row's own sequence, so
    the float64 oracle's loss is exactly 0 and every gradient exactly 0.  The step must be finite, its loss <= 1e-6 and every gradient
    zero within 1e-6 of its parameter's scale.  Negative control: the same assertion rejects 1e-5 of the scale in one SANB's fc_up.bias."""
    prob = _step_problem("down32_relu", 1)
    assert prob["loss"] == 0.0 and all(float(g.abs().max()) == 0.0 for g in prob["g"].values())

    def check(loss, grads):
        assert np.isfinite(loss) and abs(loss) <= 1e-6, loss
        for k, g in grads.items():
            assert torch.isfinite(g).all(), k
            scale = prob["P"][k].abs().max().item()
            assert g.abs().max().item() <= 1e-6 * scale, (k, g.abs().max().item(), scale)

    broken = {k: g.float() for k, g in prob["g"].items()}
    broken[ONE_SANB_BIAS] = torch.full_like(broken[ONE_SANB_BIAS], 1e-5 * prob["P"][ONE_SANB_BIAS].abs().max().item())
    assert _fails(check, 0.0, broken) and _fails(check, 2e-6, prob["g"])
    loss, grads, _, _ = _gpu_step(prob, {})
    check(loss, grads)
    print(f"hparams bs=1: loss {loss:.2e}, max |grad| / |param| {max(g.abs().max().item() / prob['P'][k].abs().max().item() for k, g in grads.items()):.2e}")


def test_mis_shaped_adapter_tensors_are_refused_before_any_launch(lib):
    """A Cached model whose cv adapter tensors were replaced by [16, 768] / [768, 16]-shaped ones (what two different
    `*_adapter_down_size` values used to build silently): `SideNetFn` raises `IisanHipError` naming the slot - the kernels would read a
    [16, 768] weight as [64, 768] and `+=` a [64, 768] gradient into it - and nothing of the side network, SASRec or the loss is launched."""
    b = synth.scientific_batch(bs=3, seed=45, item_num=N_ITEMS, res=2, words=2)
    model = helpers.build_model(helpers.make_args(drop_rate=0.0), N_ITEMS, b.pop_prob, cached=True)
    for blk in model.mm_encoder.cv_adapter_list:
        blk.fc_down.weight = torch.nn.Parameter(torch.zeros(16, 768, device="cuda"))
        blk.fc_down.bias = torch.nn.Parameter(torch.zeros(16, device="cuda"))
        blk.fc_up.weight = torch.nn.Parameter(torch.zeros(768, 16, device="cuda"))
    taps = [t[b.ids.view(-1)].cuda() for t in _tap_tables()]
    lm, ids = b.log_mask.cuda(), b.ids.view(-1).cuda()
    torch.cuda.synchronize()
    _zero_counts()
    before = _lib.dev_state(True)
    with pytest.raises(_lib.IisanHipError, match=r"slot 0 \(cv_adapter_list.0.fc_down.weight\) has shape \(16, 768\).*\(64, 768\)"):
        model(ids, taps[0].view(3, 11, 13, 768), taps[1].view(3, 11, 13, 768), lm, None)
    torch.cuda.synchronize()
    assert _lib.dev_state(True) == before, "a launch counter moved"
    assert all(v == 0 for v in _counts().values()), _counts()


# =====================================================================================================================================
# b. SASRec alone
# =====================================================================================================================================

SASREC_SEED = 987654321


@functools.lru_cache(maxsize=None)
def _sasrec_problem(B, S, H, E, L, p):
    """The recipe of `test_gpu_abi_contracts.py::_sasrec_reference` at any d_model / depth, in float64, with its float32 floor."""
    g = torch.Generator().manual_seed(1000 * E + 10 * S + B)
    pre = "user_encoder.transformer_encoder."
    shapes = {k[len(pre):]: s for k, s in weights.trainable_shapes(emb=E, seq_len=S, n_blocks=L).items() if k.startswith(pre)}
    P = weights.fill_params_seeded(shapes, seed=558)
    x = torch.randn(B, S, E, generator=g)
    lm = (torch.rand(B, S, generator=g) > 0.3).float()
    lm[:, -1] = 1
    # A query none of whose keys k <= t is a real position is attended "uniformly over all S keys" by the reference: -1e9 + score is
    # -1e9 exactly in float32 (the kernels add the same -1e9f), while float64 keeps the score - there the float64 oracle is not the
    # reference's function.  Such rows are padding positions (never a key of a real query, dropped by the loss; the float32 tests of
    # test_gpu_trainable.py hold them bit for bit): here they carry no weight in the loss and are left out of the comparison of y.
    defined = (lm.cumsum(1) > 0).float()[..., None]
    w = torch.randn(B, S, E, generator=g) * defined
    masks = None
    if p > 0:
        masks = {0: helpers.drop_factors(SASREC_SEED, 0, B * S * E, p).view(B, S, E)}
        for l in range(L):
            masks[1 + 3 * l] = helpers.drop_factors(SASREC_SEED, 1 + 3 * l, B * H * S * S, p).view(B, H, S, S)
            masks[2 + 3 * l] = helpers.drop_factors(SASREC_SEED, 2 + 3 * l, B * S * E, p).view(B, S, E)
            masks[3 + 3 * l] = helpers.drop_factors(SASREC_SEED, 3 + 3 * l, B * S * E, p).view(B, S, E)
    out = {}
    for dt in (torch.float32, torch.float64):
        Po = {k: v.to(dt).clone().requires_grad_(True) for k, v in P.items()}
        xo = x.to(dt).clone().requires_grad_(True)
        yo = O.sasrec(xo, lm.to(dt), Po, H, L, pre="", drop=None if masks is None else {s: m.to(dt) for s, m in masks.items()})
        (yo * w.to(dt)).sum().backward()
        out[dt] = dict(y=yo.detach() * defined.to(dt), dx=xo.grad.detach(), **{k: v.grad.detach() for k, v in Po.items()})
    ref = out[torch.float64]
    one_launch = E == 64 and S <= 16
    tol = {k: (2e-5 if (k == "y" or one_launch) else 1e-3) for k in ref}
    floor = {k: _fro_err(out[torch.float32][k], ref[k]) for k in ref}
    worst = max((floor[k] / tol[k], k) for k in ref)
    assert worst[0] <= 0.25, f"an ill-conditioned reference (float32 oracle vs float64 oracle {worst}): choose other inputs"
    return dict(P=P, x=x, lm=lm, w=w, defined=defined, ref=ref, tol=tol, floor=floor, one_launch=one_launch, order=ops.sasrec_param_order(L))


def _check_sasrec(got, r):
    errs = {k: _fro_err(got[k], r["ref"][k]) for k in r["ref"]}
    bad = sorted(((e / r["tol"][k], k, e) for k, e in errs.items() if not e < r["tol"][k]), reverse=True)
    assert not bad, f"{len(bad)} tensors off the float64 oracle: {bad[:4]}"
    return errs


@pytest.mark.parametrize("B,S,H,E,L,p", [(9, 12, 2, 128, 2, 0.0), (5, 16, 4, 256, 1, 0.1), (7, 32, 2, 128, 1, 0.0), (6, 1, 2, 64, 2, 0.0),
                                         (11, 32, 2, 64, 2, 0.1)])
def test_sasrec_function_at_other_widths_and_windows_matches_the_fp64_oracle(lib, B, S, H, E, L, p):
    """`SasrecFn` alone on leaf tensors: y, dx and every parameter gradient against `O.sasrec` in float64 (with dropout: the generator's
    own masks, as in `test_sasrec_dropout_matches_oracle_with_the_same_masks`).  d_model 128 / 256 is reachable through the ABI only
    (the loss and the scorer demand 64) and runs the per-operator launches, as does S = 32; S = 1 is the shortest window of the one-launch
    kernels.  Relative Frobenius: y 2e-5 everywhere, gradients 2e-5 behind the one-launch backward, 1e-3 behind the per-operator one."""
    r = _sasrec_problem(B, S, H, E, L, p)
    _check_sasrec(r["ref"], r)
    broken = dict(r["ref"])
    k0 = "transformer_blocks.0.feed_forward.w_2.bias"
    broken[k0] = torch.zeros_like(broken[k0])
    assert _fails(_check_sasrec, broken, r)                     # negative control
    cfg = ops.make_sasrec_cfg(S, E, H, L, p, SASREC_SEED)
    params = [r["P"][k].cuda().requires_grad_(True) for k in r["order"]]
    xd = r["x"].cuda().requires_grad_(True)
    _zero_counts()
    y = ops.SasrecFn.apply(cfg, xd, r["lm"].cuda(), *params)
    (y * r["w"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert _lib.dev_get("count:sasrec_fused_fwd") == (1 if r["one_launch"] else 0)
    _zero_counts()
    got = dict(y=y.detach().cpu() * r["defined"], dx=xd.grad.cpu(), **{k: t.grad.cpu() for k, t in zip(r["order"], params)})
    errs = _check_sasrec(got, r)
    wk = max(errs, key=lambda k: errs[k] / r["tol"][k])
    wg = max((k for k in errs if k not in ("y", "dx")), key=lambda k: errs[k])
    print(f"hparams sasrec B={B} S={S} H={H} E={E} L={L} p={p}: y {errs['y']:.2e} (bound 2e-05), dx {errs['dx']:.2e}, worst gradient {wg} "
          f"{errs[wg]:.2e} (bound {r['tol'][wg]:.0e}, float32 floor {r['floor'][wg]:.2e}); nearest its bound: {wk}")


def test_sasrec_refuses_windows_past_thirty_two_positions(lib):
    """The limit `check_cfg` keeps (seq x heads is no longer one of them): 33 positions are IISAN_EBADSHAPE, nothing is launched."""
    S, E, H, L = 33, 64, 2, 1
    pre = "user_encoder.transformer_encoder."
    shapes = {k[len(pre):]: s for k, s in weights.trainable_shapes(emb=E, seq_len=S, n_blocks=L).items() if k.startswith(pre)}
    P = weights.fill_params_seeded(shapes, seed=558)
    params = [P[k].cuda() for k in ops.sasrec_param_order(L)]
    _zero_counts()
    with pytest.raises(_lib.IisanHipError, match="seq 33 unsupported"):
        ops.SasrecFn.apply(ops.make_sasrec_cfg(S, E, H, L), torch.zeros(2, S, E, device="cuda"), torch.ones(2, S, device="cuda"), *params)
    torch.cuda.synchronize()
    assert all(v == 0 for v in _counts().values()), _counts()


# =====================================================================================================================================
# c. the loss alone
# =====================================================================================================================================

@functools.lru_cache(maxsize=None)
def _ce_problem(bs, S):
    """The recipe of `test_gpu_abi_contracts.py::_ce_problem` with a catalogue of at least 2 (S + 1) items (`make_ids` draws S + 1
    distinct ones per sequence)."""
    seed = bs + S
    rnd = random.Random(seed)
    lengths = [rnd.randint(2, S + 1) for _ in range(bs)]
    n = max(40, bs * 3, 2 * (S + 1))
    b = synth.scientific_batch(bs=bs, seed=90 + seed, item_num=n, res=2, words=2, lengths=lengths, dup_items=True, seq_len=S)
    g = torch.Generator().manual_seed(seed)
    score = torch.randn(bs * (S + 1), 64, generator=g) * 0.4
    prec = torch.randn(bs * S, 64, generator=g) * 0.4
    so, po = score.double().requires_grad_(True), prec.double().requires_grad_(True)
    ref = O.inbatch_ce(b.ids, so, po, b.log_mask.double(), b.pop_prob.double())
    ref.backward()
    return b, score, prec, ref.item(), so.grad.detach(), po.grad.detach()


def _check_ce(loss, d_score, d_prec, ref):
    _, _, _, loss_ref, ds_ref, dp_ref = ref
    assert abs(loss - loss_ref) <= 2e-5 * abs(loss_ref), (loss, loss_ref)
    for what, got, want in (("d_score", d_score, ds_ref), ("d_prec", d_prec, dp_ref)):
        err, scale = (_f64(got) - want).abs().max().item(), want.abs().max().item()
        assert err <= 2e-4 * scale + 1e-9, f"{what}: max|err| {err:.3e} vs scale {scale:.3e}"
    return ((_f64(d_score) - ds_ref).abs().max() / ds_ref.abs().max()).item(), ((_f64(d_prec) - dp_ref).abs().max() / dp_ref.abs().max()).item()


@pytest.mark.parametrize("bs,S", [(1, 10), (5, 1), (5, 2), (7, 16), (3, 17), (5, 31), (4, 32), (3, 63)])
def test_inbatch_ce_from_one_to_sixty_three_positions_matches_the_fp64_oracle(lib, bs, S):
    """`InbatchCeFn` on default knobs against `O.inbatch_ce` in float64: loss 2e-5 relative, both gradients within 2e-4 of their scale
    + 1e-9 (the bounds of the ragged-shape loss test).  S < 5 and S >= 16 take the generic kernel, whose `!fast` loop scans the
    sequence's ids per logit; bs = 1 leaves every row only its own label (loss 0 up to the masked logits' exp(-1e4))."""
    ref = _ce_problem(bs, S)
    b, score, prec, loss_ref, ds_ref, dp_ref = ref
    assert lib.iisan_inbatch_ce_route(bs, S) == (0 if (S < 5 or S >= 16) else 2)
    _check_ce(loss_ref, ds_ref, dp_ref, ref)
    if bs > 1:                                                  # negative control: the row of d_score that holds its largest element, zeroed
        broken = ds_ref.clone()
        broken[int(ds_ref.abs().max(1).values.argmax())] = 0
        assert _fails(_check_ce, loss_ref, broken, dp_ref, ref) and _fails(_check_ce, loss_ref * (1 + 1e-4), ds_ref, dp_ref, ref)
    sd, pd = score.cuda().requires_grad_(True), prec.cuda().requires_grad_(True)
    loss = ops.InbatchCeFn.apply(b.ids.view(-1).cuda(), sd, pd, b.log_mask.cuda(), b.pop_prob.cuda())
    loss.backward()
    torch.cuda.synchronize()
    if bs == 1:     # the oracle: exactly 0 and zero gradients
        assert loss_ref == 0.0 and float(ds_ref.abs().max()) == 0.0
        assert abs(loss.item()) <= 1e-6 and sd.grad.abs().max().item() <= 1e-9 and pd.grad.abs().max().item() <= 1e-9
        return
    e = _check_ce(loss.item(), sd.grad, pd.grad, ref)
    print(f"hparams ce bs={bs} S={S}: loss {abs(loss.item() - loss_ref) / abs(loss_ref):.1e}, d_score {e[0]:.2e}, d_prec {e[1]:.2e} (bound 2e-4)")


@pytest.mark.parametrize("S", [0, 64])
def test_inbatch_ce_refuses_windows_outside_one_to_sixty_three_without_launching(lib, S):
    """`iisan_inbatch_ce_fwd` at S = 0 and S = 64: IISAN_EBADSHAPE, and neither the loss nor the workspace is written."""
    bs = 3
    assert lib.iisan_inbatch_ce_route(bs, S) < 0
    ids = torch.ones(bs * (S + 1), dtype=torch.int64, device="cuda")
    score = torch.zeros(bs * (S + 1), 64, device="cuda")
    prec = torch.zeros(max(bs * S, 1), 64, device="cuda")
    lm = torch.ones(bs, max(S, 1), device="cuda")
    pop = torch.ones(8, device="cuda")
    loss = torch.full((4,), float("nan"), device="cuda")
    ws = torch.full((max(int(lib.iisan_inbatch_ce_ws_bytes(bs, S)), 0) + (1 << 20),), 0xA5, dtype=torch.uint8, device="cuda")
    tok = C.c_uint64(0)
    rc = lib.iisan_inbatch_ce_fwd(ids.data_ptr(), score.data_ptr(), prec.data_ptr(), lm.data_ptr(), pop.data_ptr(), pop.numel(), bs, S, 64,
                                  loss.data_ptr(), ws.data_ptr(), ws.numel(), C.byref(tok), _stream())
    torch.cuda.synchronize()
    assert rc == IISAN_EBADSHAPE and b"unsupported" in lib.iisan_last_error()
    assert tok.value == 0 and bool(torch.isnan(loss).all()) and bool((ws == 0xA5).all())


# =====================================================================================================================================
# d. eval at a non-default window
# =====================================================================================================================================

def _pack_window(seqs, S, first=False):
    """The reference's eval rows (`Code_Uncached/data_utils/dataset.py:183-189`): the LAST S history items, left padded.  `first`: the
    first S instead - the wrong truncation of the negative controls."""
    tok, lm = torch.zeros(len(seqs), S, dtype=torch.int64), torch.zeros(len(seqs), S)
    for u, seq in enumerate(seqs):
        t = (seq[:-1][:S] if first else seq[:-1][-S:])
        tok[u, S - len(t):] = torch.tensor(t)
        lm[u, S - len(t):] = 1
    return tok, lm


def _check_eval(model, item_emb, seqs, S, H, L, P_user, tol):
    """ranks / top-10 lists bit-equal to the oracle's on the product's own user vectors; the user vectors within `tol` (relative
    Frobenius, float64 oracle) of `O.sasrec` on the host-packed window; both rejected on the wrongly truncated window."""
    hists = [s[:-1] for s in seqs]
    tgt = torch.tensor([s[-1] for s in seqs])
    ranks = evaluate.evaluate_ranks(model, item_emb, seqs, hists, max_seq_len=S).cpu().long()
    top, _ = evaluate.recommend_topk(model, item_emb, hists, hists, max_seq_len=S, k=10)
    tok, lm = _pack_window(seqs, S)
    model.eval()
    with torch.no_grad():
        prec = model.user_encoder(item_emb[tok.cuda()], lm.cuda(), None)[:, -1].contiguous().cpu()
    emb = item_emb.cpu()
    ht = [torch.tensor(h) for h in hists]
    assert torch.equal(ranks, O.eval_ranks(prec, emb, ht, tgt))
    assert torch.equal(top.cpu().long(), O.eval_topk(prec, emb, ht, 10))
    Pd = {k: v.double() for k, v in P_user.items()}
    want = O.sasrec(emb.double()[tok], lm.double(), Pd, H, L)[:, -1]
    err = _fro_err(prec, want)
    assert err < tol, err
    # negative controls: the first S items instead of the last S
    tok_w, lm_w = _pack_window(seqs, S, first=True)
    assert not torch.equal(tok_w, tok), "no history is longer than the window"
    wrong = O.sasrec(emb.double()[tok_w], lm_w.double(), Pd, H, L)[:, -1]
    assert not _fro_err(prec, wrong) < tol
    assert not torch.equal(ranks, O.eval_ranks(wrong.float(), emb, ht, tgt))
    return err


def test_eval_at_a_window_of_twenty_positions_truncates_long_histories_like_the_reference(lib):
    """A Cached model with `max_seq_len` 20, one block, four heads (80 = seq x heads: the per-operator SASRec launches), seeded parameters;
    the item table is the model's own (`evaluate.item_table` over 301 rows of synthetic taps); 64 users with 2 .. 30 items, so a third of
    the histories are longer than the window, every seventh user a repeat purchase."""
    S, H, L, n = 20, 4, 1, 300
    args = helpers.make_args(drop_rate=0.0, max_seq_len=S, transformer_block=L, num_attention_heads=H)
    model = helpers.build_model(args, n, synth.make_pop_prob(n), cached=True)
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters() if p.requires_grad}
    P = weights.fill_params_seeded(shapes, seed=559)
    helpers.load_trainables(model, P)
    ids = torch.arange(n + 1)
    with torch.no_grad():
        item_emb = evaluate.item_table(model, synth.cached_taps(ids, 12, 768, seed=35).cuda(), synth.cached_taps(ids, 12, 768, seed=36).cuda())
    assert item_emb.shape == (n + 1, 64)
    rs = np.random.RandomState(6)
    seqs = []
    for u in range(64):
        l = 2 + (u * 28) // 63                           # 2 .. 30, every length region covered
        seq = [int(x) for x in rs.choice(np.arange(1, n + 1), size=l, replace=False)]
        if u % 7 == 0 and l > 2:
            seq[-1] = seq[0]                             # repeat purchase: the target sits in its own history (outside the window when l > 21)
        seqs.append(seq)
    assert max(len(s) for s in seqs) == 30 and sum(len(s) - 1 > S for s in seqs) >= 16
    err = _check_eval(model, item_emb, seqs, S, H, L, {k: v for k, v in P.items() if k.startswith("user_encoder.")}, 2e-5)
    print(f"hparams eval S=20 H=4 L=1: prec {err:.2e} (bound 2e-5)")


def test_eval_at_a_window_of_five_positions_on_the_eval_fixture(lib):
    """The sequences of `tests/golden/eval.npz` (up to 11 items) through a `max_seq_len` 5 user encoder: most histories are truncated."""
    from iisan_amd.model import User_Encoder
    z, seqs, tables, P = gio.eval_inputs()
    S = 5
    item_emb = ops.LinearFn.apply(torch.cat(tables, 1).cuda(), P["com_dense.weight"].cuda(), P["com_dense.bias"].cuda())
    pos = "user_encoder.transformer_encoder.position_embedding.weight"
    Pu = {k: (v[:S].clone() if k == pos else v) for k, v in P.items() if k.startswith("user_encoder.")}

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.user_encoder = User_Encoder(int(z["item_num"]), S, 64, 2, 0.1, 2)

    model = Holder().cuda()
    model.user_encoder.load_state_dict({k[len("user_encoder."):]: v for k, v in Pu.items()})
    assert sum(len(s) - 1 > S for s in seqs) >= 10
    err = _check_eval(model, item_emb, seqs, S, 2, 2, Pu, 2e-5)
    print(f"hparams eval S=5 H=2 L=2: prec {err:.2e} (bound 2e-5)")
