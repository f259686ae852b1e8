"""The whole model at `embedding_dim` 128, 192 and 256 - the launcher argument every layer follows: the side network's heads, `com_dense`,
SASRec on its per-operator launches (d_model > 64), the in-batch loss on its f32 routes, and the eval path on the same models.

Training step: one Cached step exactly as `test_gpu_hparams.py::test_cached_step_at_non_default_hyperparameters_matches_the_fp64_oracle`
runs it - that file's batch maker, tap tables, `O.model_loss_from_taps` in float64, `_check_step`'s bounds and its conditioning guard
(the float32 oracle within a quarter of every bound).  Eval: `evaluate.evaluate_ranks` / `recommend_topk` against `O.eval_ranks` /
`O.eval_topk` on the product's own float32 user vectors, `evaluate.eval_model`'s Hit@10 against `O.hit_ndcg` of those ranks.
Measured errors: `profiles/wide_embedding.md`."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers  # noqa: E402
from iisan_amd import evaluate, synth, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402
from test_gpu_hparams import (CACHED_HEADS, N_ITEMS, ONE_SANB_BIAS, _case, _check_step, _fails, _gpu_step, _lengths, _report,  # noqa: E402
                              _step_errors, _tap_tables)

WIDE_CASES = {
    "emb128_h2": dict(_case(H=2), embedding_dim=128),
    "emb128_h2_gelu": dict(_case(H=2, act="GELU"), embedding_dim=128),
    "emb192_h3": dict(_case(H=3), embedding_dim=192),
    "emb256_h4": dict(_case(H=4), embedding_dim=256),
    "emb256_h4_s16_down32_gelu": dict(_case(H=4, S=16, down=32, act="GELU"), embedding_dim=256),
}
# Batch seed per (case, batch size), as `STEP_SEEDS` of test_gpu_hparams.py: 45 unless that batch's reference is ill-conditioned (the
# first seed from 45 on whose float32 oracle stays within a quarter of every bound of the float64 one - a property of the reference alone)
# (45 at 256 / S = 16 / bs 37: the float32 oracle is 1.6e-2 off the float64 one on block 0's w_1 - 8 x the bound - when torch runs it on
#  16 threads, and 0.006 of the bound on 8: a reference that depends on the reduction order of the host's GEMM is not one to test against)
STEP_SEEDS = {("emb256_h4_s16_down32_gelu", 37): 46}


@functools.lru_cache(maxsize=None)
def _step_problem(case, bs):
    return _build(case, bs, STEP_SEEDS.get((case, bs), 45))


def _build(case, bs, SEED):
    """`test_gpu_hparams.py::_step_problem` for a case of WIDE_CASES: batch, seeded parameters, the float64 oracle's loss and gradients,
    and the conditioning check of the reference itself.  Computed once per (case, batch size), never modified."""
    kw = WIDE_CASES[case]
    S, act = kw["max_seq_len"], kw["adapter_activation"]
    b = synth.scientific_batch(bs=bs, seed=SEED, seq_len=S, item_num=N_ITEMS, res=2, words=2, lengths=_lengths(bs, S, SEED), dup_items=True)
    real = (b.ids != 0).sum(1)
    assert int(real.max()) == S + 1 and int(real.min()) == 2
    args = helpers.make_args(drop_rate=0.0, **kw)
    shapes = {k: tuple(p.shape) for k, p in helpers.build_model(args, N_ITEMS, b.pop_prob, cached=True, device="cpu").named_parameters()
              if p.requires_grad}
    assert shapes["com_dense.weight"][0] == kw["embedding_dim"]
    P = weights.fill_params_seeded(shapes, seed=557)
    layers = O.side_layer_list(kw["side_adapter_vit_list"], False)
    tabs = _tap_tables()
    ids = b.ids.view(-1)
    out = {}
    for dt in (torch.float32, torch.float64):
        Po = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in P.items()}
        loss, _ = O.model_loss_from_taps(ids, tabs[0][ids].to(dt), tabs[1][ids].to(dt), b.log_mask.to(dt), b.pop_prob.to(dt), Po, layers,
                                         heads=kw["num_attention_heads"], n_layers=kw["transformer_block"], activation=act,
                                         fusion=kw["fusion_method"], remove_first=False, **CACHED_HEADS)
        loss.backward()
        out[dt] = (loss.item(), {k: v.grad.detach() for k, v in Po.items()})
    loss, grads = out[torch.float64]
    prob = dict(case=case, bs=bs, kw=kw, act=act, b=b, P=P, loss=loss, g=grads)
    prob["floor"] = _step_errors(out[torch.float32][1], grads, act)
    worst = max((e / tol, k, e) for k, (e, tol) in prob["floor"].items())
    assert worst[0] <= 0.25, f"an ill-conditioned reference (float32 oracle vs float64 oracle, error / bound {worst}): choose another batch"
    return prob


@pytest.mark.parametrize("bs", [3, 37])
@pytest.mark.parametrize("case", list(WIDE_CASES))
def test_cached_step_at_wide_embedding_dims_matches_the_fp64_oracle(lib, case, bs):
    """One Cached training step (tap stores, default knobs) at `embedding_dim` 128 / 192 / 256 against the float64 oracle on the same
    taps and parameters: loss 2e-5 relative, every gradient within `_check_step`'s bound.  Counters: SASRec on its per-operator
    launches, no split-operand loss pass; the loss route is what `iisan_inbatch_ce_route_e` says (fused at S = 10, generic at S = 16)."""
    prob = _step_problem(case, bs)
    kw = prob["kw"]
    E, S = kw["embedding_dim"], kw["max_seq_len"]
    _check_step(prob["loss"], prob["g"], prob)
    broken = dict(prob["g"])
    broken[ONE_SANB_BIAS] = torch.zeros_like(broken[ONE_SANB_BIAS])
    assert _fails(_check_step, prob["loss"], broken, prob)
    assert _fails(_check_step, prob["loss"] * (1 + 1e-4), prob["g"], prob)
    loss, grads, c, model = _gpu_step(prob, {})
    assert model.com_dense.weight.shape[0] == E
    errs = _check_step(loss, grads, prob)
    _report(f"wide {case} bs={bs} loss {abs(loss - prob['loss']) / abs(prob['loss']):.1e}", errs)
    assert c["sasrec_fused_fwd"] == 0 and c["ce16"] == 0, c
    assert lib.iisan_inbatch_ce_route_e(bs, S, E) == (0 if S >= 16 else 2)


@pytest.mark.parametrize("case", ["emb128_h2", "emb256_h4"])
def test_eval_on_a_wide_model_matches_the_oracle_on_its_own_user_vectors(lib, case):
    """A Cached model at `embedding_dim` 128 / 256 with seeded parameters, its own item table (`evaluate.item_table` over 301 rows of
    synthetic taps), 40 users with 2 .. 25 items (windows shorter and longer than `max_seq_len` 10), every seventh a repeat purchase:
    ranks and top-10 lists bit-equal to `O.eval_ranks` / `O.eval_topk` on the product's own user vectors, the user vectors within 2e-5
    (relative Frobenius) of `O.sasrec` in float64, `eval_model`'s Hit@10 equal to `O.hit_ndcg` of those ranks."""
    kw = WIDE_CASES[case]
    E, S, H, L, n = kw["embedding_dim"], kw["max_seq_len"], kw["num_attention_heads"], kw["transformer_block"], 300
    args = helpers.make_args(drop_rate=0.0, **kw)
    model = helpers.build_model(args, n, synth.make_pop_prob(n), cached=True)
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters() if p.requires_grad}
    P = weights.fill_params_seeded(shapes, seed=559)
    helpers.load_trainables(model, P)
    ids = torch.arange(n + 1)
    cv, tx = synth.cached_taps(ids, 12, 768, seed=35).cuda(), synth.cached_taps(ids, 12, 768, seed=36).cuda()
    with torch.no_grad():
        item_emb = evaluate.item_table(model, cv, tx)
        item3, _ = model.mm_encoder.forward_item3(cv, tx)
    assert item_emb.shape == (n + 1, E) and item3.shape == (n + 1, 3 * E)
    rs = np.random.RandomState(6)
    seqs = []
    for u in range(40):
        l = 2 + (u * 23) // 39
        seq = [int(x) for x in rs.choice(np.arange(1, n + 1), size=l, replace=False)]
        if u % 7 == 0 and l > 2:
            seq[-1] = seq[0]
        seqs.append(seq)
    assert max(len(s) for s in seqs) == 25 and sum(len(s) - 1 > S for s in seqs) >= 10 and sum(len(s) - 1 < S for s in seqs) >= 10
    hists = [s[:-1] for s in seqs]
    tgt = torch.tensor([s[-1] for s in seqs])
    ranks = evaluate.evaluate_ranks(model, item_emb, seqs, hists, max_seq_len=S).cpu().long()
    top, _ = evaluate.recommend_topk(model, item_emb, hists, hists, max_seq_len=S, k=10)
    tok, lm = torch.zeros(len(seqs), S, dtype=torch.int64), torch.zeros(len(seqs), S)
    for u, seq in enumerate(seqs):
        t = seq[:-1][-S:]
        tok[u, S - len(t):] = torch.tensor(t)
        lm[u, S - len(t):] = 1
    model.eval()
    with torch.no_grad():
        prec = model.user_encoder(item_emb[tok.cuda()], lm.cuda(), None)[:, -1].contiguous().cpu()
    emb = item_emb.cpu()
    ht = [torch.tensor(h) for h in hists]
    want_ranks = O.eval_ranks(prec, emb, ht, tgt)
    assert torch.equal(ranks, want_ranks)
    assert torch.equal(top.cpu().long(), O.eval_topk(prec, emb, ht, 10))
    Pd = {k: v.double() for k, v in P.items() if k.startswith("user_encoder.")}
    want = O.sasrec(emb.double()[tok], lm.double(), Pd, H, L)[:, -1]
    err = ((prec.double() - want).norm() / want.norm()).item()
    assert err < 2e-5, err
    # negative control: the scores of the first 64 features alone rank otherwise
    assert not torch.equal(ranks, O.eval_ranks(prec[:, :64].contiguous(), emb[:, :64].contiguous(), ht, tgt))

    class Log:
        lines = []

        def info(self, msg):
            self.lines.append(msg)

    hit = evaluate.eval_model(model, {u: torch.tensor(h) for u, h in enumerate(hists)}, dict(enumerate(seqs)), item3[:, :E].contiguous(),
                              [item3[:, E:2 * E].contiguous(), item3[:, 2 * E:].contiguous()], 16, args, n, Log(), "validation", 0)
    want_hit, _ = O.hit_ndcg(want_ranks, 10)
    assert abs(float(hit) - float(want_hit.mean())) < 1e-9, (hit, want_hit.mean())
    print(f"wide eval {case}: prec {err:.2e} (bound 2e-5), Hit@10 {float(hit):.4f}, ranks and top-10 lists bit-equal to the oracle's")
