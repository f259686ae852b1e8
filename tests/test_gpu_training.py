"""Training past the first Adam step: the fused Adam kernel against float64 Adam at any step, and K-step trajectories of
`FlatTrainer` against the same K steps of the float64 CPU oracle (`oracle/iisan_oracle.py`, pinned to the reference by the
golden fixtures): loss at every step, every trainable tensor's displacement, the Adam moments, a resumed checkpoint of a stock
`torch.optim.Adam`, and the ranks the trained model gives.

At step 1 from zero moments Adam's update is `lr * g / (|g| + eps)` whatever beta1, beta2 and the moments are, so every test
that stops there would pass a kernel that never writes `m` / `v` back or a bias correction stuck at step 1.  Here every
comparison runs step >= 2 with real moments.

Trajectory metric (per trainable tensor, float64): `|(p_K - p_0) - (p_K_ref - p_0)| / |p_K_ref - p_0|` in the Frobenius norm —
ReLU unit flips make single-element bounds meaningless (see the bench-size oracle test of test_gpu_trainable.py); the one-scalar
gates of a tower are held together as the vector they form.  The moments are held in the same norm.  The float64 oracle gets
the fp32 tap values the device reads, so the trajectories differ by the fp32 arithmetic of the device alone; its measured size
on the host (fp32 oracle against float64 oracle, same setup) is ~1.6e-4 worst tensor with ReLU adapters, ~1.2e-3 with GELU,
while a broken optimiser moves every tensor by more than 1e-2 (`test_trajectory_comparison_rejects_a_broken_optimiser`)."""
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import golden_io as gio  # noqa: E402
import helpers  # noqa: E402
from iisan_amd import _lib, evaluate, ops, synth, tapstore, trainer, weights  # noqa: E402
from oracle import iisan_oracle as O  # noqa: E402

F32 = lambda x: float(np.float32(x))        # noqa: E731  the value an fp32 argument of the C ABI holds
B1, B2, EPS = F32(0.9), F32(0.999), F32(1e-8)


# ---------------------------------------------------------------------------------------------------------------
# A.  iisan_adam_step against float64 Adam, past step one
# ---------------------------------------------------------------------------------------------------------------

def _ulp(x):
    """fp32 unit in the last place of |x| (float64 tensor in, float64 tensor out; 2^-149 at zero)."""
    e = torch.frexp(x.abs()).exponent
    return torch.ldexp(torch.ones_like(x), (e - 24).clamp(min=-149))


def _lr_per_element(n, seg_end, seg_lr):
    lr = torch.empty(n, dtype=torch.float64)
    lo = 0
    for e, l in zip(seg_end, seg_lr):
        lr[lo:e] = F32(l)
        lo = e
    return lr


def _adam_ref(p, g, m, v, seg_end, seg_lr, step, gs):
    """One step of the oracle's Adam (`O.adam_step`, torch.optim.Adam's formula) in float64 on the fp32 inputs, with the
    constants the kernel receives (beta1, beta2, eps and the rates are fp32 arguments of the ABI).  Returns (p, m, v) and the
    per-element bounds of the kernel's fp32 arithmetic: m and v a few fp32 ulp of the sums that form them (m may cancel), p one
    fp32 ulp plus 1e-5 of the update plus what the m bound moves the update by."""
    p, g, m, v = (t.detach().cpu().double() for t in (p, g, m, v))
    g = g * gs
    lr = _lr_per_element(p.numel(), seg_end, seg_lr)
    p2, m2, v2 = O.adam_step(p, g, m, v, step, lr, B1, B2, EPS)
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    denom = (v2 / bc2).sqrt() + EPS
    tol_m = 3 * _ulp(B1 * m.abs() + (1 - B1) * g.abs())
    tol_v = 4 * _ulp(B2 * v + (1 - B2) * g * g)
    tol_p = _ulp(p2) + 1e-5 * (p2 - p).abs() + lr / bc1 * tol_m / denom
    return (p2, m2, v2), (tol_p, tol_m, tol_v)


def _adam_kernel_check(p, g, m, v, seg_end, seg_lr, step, gs, what):
    """Run the kernel once on device copies, check p / m / v per element, return the new device state and the worst
    error-to-bound ratios."""
    (pr, mr, vr), (tp, tm, tv) = _adam_ref(p, g, m, v, seg_end, seg_lr, step, gs)
    ops.adam_step(p, g, m, v, seg_end, seg_lr, step, grad_scale=gs)
    torch.cuda.synchronize()
    worst = {}
    for name, got, ref, tol in (("p", p, pr, tp), ("m", m, mr, tm), ("v", v, vr, tv)):
        err = (got.cpu().double() - ref).abs()
        ratio = (err / tol).max().item()
        worst[name] = ratio
        bad = int((err > tol).sum())
        assert bad == 0, f"{what}: {name} off at {bad} elements, worst err/bound {ratio:.2f}"
    return worst


def _adam_inputs(n, seed, g_scale=1.0, dev="cuda"):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * g_scale
    m = torch.randn(n, generator=gen) * 0.3 * g_scale
    v = (torch.randn(n, generator=gen) * g_scale) ** 2
    return [t.to(dev) for t in (p, g, m, v)]


_SEG_CASES = {
    "n1": (1, [1]),
    "n255": (255, [255]),
    "n257_2seg": (257, [100, 257]),
    "ragged_5seg": (70001, [13, 257, 40000, 40001, 70001]),          # boundaries off every multiple of 256, a 1-element segment
    "ragged_8seg": (10007, [1, 300, 513, 513, 1000, 5000, 9999, 10007]),   # the maximum segment count, one empty segment
}
_SEG_LRS = [1e-3, 3e-3, 2e-4, 7e-3, 5e-4, 9e-3, 4e-3, 6e-4]              # distinct: a neighbour segment's rate fails the test


@pytest.mark.parametrize("step", [2, 3, 10, 1000, 10 ** 6])
@pytest.mark.parametrize("case", sorted(_SEG_CASES))
def test_adam_kernel_past_step_one_matches_float64(case, step):
    n, seg_end = _SEG_CASES[case]
    seg_lr = _SEG_LRS[:len(seg_end)]
    for gs in (1.0, 0.5, 0.125):
        p, g, m, v = _adam_inputs(n, seed=n + step)
        _adam_kernel_check(p, g, m, v, seg_end, seg_lr, step, gs, f"{case} step {step} grad_scale {gs}")


@pytest.mark.parametrize("step", [2, 1000])
def test_adam_kernel_at_the_trainer_flat_size(step):
    """The real flat buffer of the Cached IISAN trainer (5 Adam groups, alignment padding): n is above 4096 * 256, so every
    thread of the capped grid runs the grid-stride loop more than once."""
    args = helpers.make_args(drop_rate=0.0)
    model = helpers.build_model(args, 30, synth.make_pop_prob(30), cached=True)
    tr = trainer.FlatTrainer(model, args)
    n = tr.flat.numel()
    assert n > 4096 * 256 and len(tr.seg_end) == 5 and tr.seg_end[-1] == n
    seg_lr = [1e-4, 2e-4, 3e-4, 4e-4, 5e-4]
    p, g, m, v = _adam_inputs(n, seed=step)
    _adam_kernel_check(p, g, m, v, tr.seg_end, seg_lr, step, 0.5, f"trainer size step {step}")


def test_adam_kernel_gradient_extremes():
    """Gradients near eps (the update is then eps-dominated) and around 1e3, in one buffer, over several steps."""
    n = 4099
    gen = torch.Generator().manual_seed(8)
    for step in (2, 7, 50):
        p = torch.randn(n, generator=gen)
        g = torch.cat([torch.randn(n // 2, generator=gen) * 1e-8, torch.randn(n - n // 2, generator=gen) * 1e3])
        m = g * torch.rand(n, generator=gen)
        v = g * g * (1 + torch.rand(n, generator=gen))
        p, g, m, v = (t.cuda() for t in (p, g, m, v))
        _adam_kernel_check(p, g, m, v, [1000, n], [1e-3, 2e-4], step, 1.0, f"extremes step {step}")


def test_adam_kernel_thirty_steps_on_its_own_moments():
    """30 steps, each fed the kernel's own p / m / v of the step before and a fresh gradient: every step is checked per element
    (a kernel that does not write m / v back fails its next step), and the 30-step trajectory stays with an independent
    float64 trajectory of the same gradients (no compounding)."""
    n, seg_end = _SEG_CASES["ragged_5seg"]
    seg_lr = _SEG_LRS[:5]
    p, _, m, v = _adam_inputs(n, seed=3)
    m.zero_()
    v.zero_()
    p0 = p.cpu().double()
    pr, mr, vr = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    lr = _lr_per_element(n, seg_end, seg_lr)
    gen = torch.Generator().manual_seed(4)
    for step in range(1, 31):
        g = (torch.randn(n, generator=gen) + 0.3).cuda()         # a bias, so that the moments carry a signal across steps
        gs = (1.0, 0.5, 0.125)[step % 3]
        _adam_kernel_check(p, g, m, v, seg_end, seg_lr, step, gs, f"loop step {step}")
        pr, mr, vr = O.adam_step(pr, g.cpu().double() * gs, mr, vr, step, lr, B1, B2, EPS)
    rel = {name: ((got.cpu().double() - ref).norm() / (ref - base).norm()).item()
           for name, got, ref, base in (("p", p, pr, p0), ("m", m, mr, 0), ("v", v, vr, 0))}
    print(f"measured: adam 30-step trajectory rel p {rel['p']:.2e} m {rel['m']:.2e} v {rel['v']:.2e}")
    # p itself is stored in fp32: each step rounds it by up to half an ulp (1.2e-7 at |p| ~ 1), a random walk that reaches ~1e-4
    # of the 30 steps' displacement of the 2e-4 segment (measured on MI355X: 3.8e-5); the moments do not accumulate
    assert rel["p"] < 1.5e-4 and rel["m"] < 1e-6 and rel["v"] < 1e-6, rel


def test_adam_kernel_keeps_the_alignment_padding_at_zero():
    """Elements with g = m = v = p = 0 (the trainer's alignment padding) stay exactly zero over many steps, between live
    elements of every segment."""
    n, seg_end = _SEG_CASES["ragged_8seg"]
    p, g, m, v = _adam_inputs(n, seed=9)
    pad = torch.zeros(n, dtype=torch.bool)
    pad[5::16] = True
    pad[seg_end[0] - 1] = True
    for t in (p, m, v):
        t[pad.cuda()] = 0
    gen = torch.Generator().manual_seed(10)
    for step in range(1, 41):
        g.copy_(torch.randn(n, generator=gen))
        g[pad.cuda()] = 0
        ops.adam_step(p, g, m, v, seg_end, _SEG_LRS, step, grad_scale=0.5)
    for t in (p, m, v):
        assert torch.equal(t.cpu()[pad], torch.zeros(int(pad.sum())))
    assert (p.cpu()[~pad] != 0).all()


def test_adam_argument_checks():
    """`seg_end` must give every element exactly one segment: non-decreasing from 0, last end == n (include/iisan_hip.h)."""
    n = 1000
    p, g, m, v = _adam_inputs(n, seed=1)
    before = p.clone()
    for seg_end in ([999], [1001], [600, 300, 1000], [-1, 1000], [500, 999], [1000, 999]):
        with pytest.raises(_lib.IisanHipError):
            ops.adam_step(p, g, m, v, seg_end, [1e-3] * len(seg_end), 2)
    for n_seg in (0, 9):
        with pytest.raises(_lib.IisanHipError):
            ops.adam_step(p, g, m, v, [n] * n_seg, [1e-3] * n_seg, 2)
    with pytest.raises(_lib.IisanHipError):
        ops.adam_step(p, g, m, v, [n], [1e-3], 0)
    torch.cuda.synchronize()
    assert torch.equal(p, before)                               # nothing was launched
    ops.adam_step(p, g, m, v, [0, 0, 400, 400, n], [1e-3] * 5, 2)     # empty segments are allowed
    torch.cuda.synchronize()
    assert not torch.equal(p, before)


# ---------------------------------------------------------------------------------------------------------------
# B.  K-step trajectories: FlatTrainer against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------

CACHED_LIST = "0,1,2,3,4,5"            # 7 taps (layers 0..6) with layer 0; 6 taps + the seeding tap 0 with remove_first


@dataclass
class Case:
    kind: str                          # "cached" | "versa" | "uncached"
    bs: int
    steps: int
    act: str = "RELU"
    rmfirst: bool = False
    items: int = 300                   # catalogue size (a 40-item catalogue made the Uncached case ill-conditioned: fp32 floor 1e-2)
    drop: float = 0.0
    extra: dict = field(default_factory=dict)


# One bound for every case: 3-4x the worst value measured on MI355X over all cases and runs.  The worst tensor is decided by
# ReLU unit flips that differences at the 1e-7 level (the device's summation order; not bitwise repeatable between processes)
# set off, so it moves between runs: measured worst loss / tensor displacement / moment per case, over three runs —
#   cached_relu_bs16 1.1e-6 / 1.2e-4 / 7.2e-5     cached_gelu_rmfirst_bs16 7.0e-7 / 5.6e-4 / 1.6e-5
#   cached_relu_bs128 5.5e-7 / 4.5e-4 / 3.8e-4    cached_relu_bs1024 8.1e-7 / 8.1e-4 / 7.1e-4
#   versa_bs16 5.5e-7 / 1.6e-3 / 2.6e-3          uncached_bs8 1.4e-6 / 2.9e-4 / 6.5e-4
#   cached_relu_bs16_dropout 7.2e-7 / 9.0e-4 / 1.5e-3
BOUND_LOSS, BOUND_P, BOUND_MV = 5e-6, 5e-3, 8e-3
CASES = {
    "cached_relu_bs16": Case("cached", 16, 24),
    "cached_gelu_rmfirst_bs16": Case("cached", 16, 24, act="GELU", rmfirst=True),
    "cached_relu_bs128": Case("cached", 128, 8, items=2000),
    "cached_relu_bs1024": Case("cached", 1024, 5, items=2000),
    "versa_bs16": Case("versa", 16, 16, extra=dict(Di=256, Dt=512, Lc=6, Lt=10, vlist="0,2,4", blist="1,3,5,7,8")),
    "uncached_bs8": Case("uncached", 8, 12),
    "cached_relu_bs16_dropout": Case("cached", 16, 16, drop=0.1),
}


class Setup:
    """Product model + trainer on the device, seeded parameters, the catalogue's taps, and the oracle's view of the same."""

    def __init__(self, case: Case, device="cuda"):
        self.case = c = case
        self.pop = synth.make_pop_prob(c.items)
        if c.kind == "cached":
            self.args = helpers.make_args(drop_rate=c.drop, adapter_activation=c.act, side_adapter_vit_list=CACHED_LIST,
                                          side_adapter_bert_list=CACHED_LIST, remove_first="TRUE" if c.rmfirst else "None")
            self.model = helpers.build_model(self.args, c.items, self.pop, cached=True, device=device)
            g = torch.Generator().manual_seed(5)
            self.tabs = [torch.randn(c.items + 1, 7, 768, generator=g) * 0.25 for _ in range(2)]
            for t in self.tabs:
                t[0] = 0
            lay = self.model.mm_encoder.packed_layers()
            assert lay == list(range(7)) or lay == [0] + list(range(1, 7))
            if device == "cuda":
                self.model.tap_stores = tuple(tapstore.TapStore(t.cuda(), lay, "cuda", "fp32") for t in self.tabs)
            self.layers = O.side_layer_list(CACHED_LIST, c.rmfirst)
        elif c.kind == "versa":
            x = c.extra
            self.args = helpers.make_args(drop_rate=c.drop, adapter_activation=c.act, text_embedding_dim=x["Dt"],
                                          image_embedding_dim=x["Di"], side_adapter_vit_list=x["vlist"],
                                          side_adapter_bert_list=x["blist"], image_layers=x["Lc"] - 1, text_layers=x["Lt"] - 1)
            self.model = helpers.build_model(self.args, c.items, self.pop, cached="versa", device=device)
            g = torch.Generator().manual_seed(6)
            self.tabs = [torch.randn(c.items + 1, x["Lc"], x["Di"], generator=g) * 0.25,
                         torch.randn(c.items + 1, x["Lt"], x["Dt"], generator=g) * 0.25]
            for t in self.tabs:
                t[0] = 0
            self.layers = (O.side_layer_list(x["vlist"], False), O.side_layer_list(x["blist"], False))
        else:
            self.args = helpers.make_args(drop_rate=c.drop, side_adapter_vit_list="0,1", side_adapter_bert_list="0,1",
                                          num_words_title=8)
            vw, bw = weights.make_vit_weights(gio.E2E_VIT, seed=11), weights.make_bert_weights(gio.E2E_BERT, seed=12)
            self.model = helpers.build_model(self.args, c.items, self.pop, vw, gio.E2E_VIT, bw, gio.E2E_BERT, cached=False)
            ids = np.arange(c.items + 1)
            self.cat_img = synth.make_images(ids, 32, seed=21).cuda()            # one picture and one title per item, row 0 = padding
            self.cat_txt = torch.from_numpy(synth.make_text(ids, 8, 512, np.random.RandomState(22))).cuda()
            tc, tt = evaluate.build_tap_cache(self.model, self.cat_img, self.cat_txt)
            self.tabs = [tc.cpu(), tt.cpu()]
            self.layers = O.side_layer_list("0,1", False)
        shapes = {n: tuple(p.shape) for n, p in self.model.named_parameters() if p.requires_grad}
        self.P = weights.fill_params_seeded(shapes, seed=557)
        helpers.load_trainables(self.model, self.P)
        self.model.train()
        self.heads = (dict(cv_head="mm_encoder.cv_pre_fc.", text_head="mm_encoder.bert_pre_fc.") if c.kind == "cached" else {})

    def batch(self, k):
        return synth.scientific_batch(bs=self.case.bs, seed=900 + k, item_num=self.case.items, res=2, words=2)

    def device_inputs(self, b):
        ids = b.ids.view(-1)
        if self.case.kind == "cached":
            return ids.cuda(), None, None
        if self.case.kind == "uncached":
            return ids.cuda(), self.cat_img[ids.cuda()], self.cat_txt[ids.cuda()]
        bs, S1 = b.ids.shape
        return (ids.cuda(), self.tabs[0][ids].view(bs, S1, *self.tabs[0].shape[1:]).cuda(),
                self.tabs[1][ids].view(bs, S1, *self.tabs[1].shape[1:]).cuda())

    def oracle_loss(self, P, b, drop=None):
        """The oracle's loss on float64 copies of the taps the device reads (model_loss_from_taps composed, so that the
        SASRec dropout masks can be passed in)."""
        c = self.case
        ids = b.ids.view(-1)
        tc, tt = self.tabs[0][ids].double(), self.tabs[1][ids].double()
        lm, pop = b.log_mask.double(), self.pop.double()
        bs, S = b.log_mask.shape
        if c.kind == "versa":
            cv, text, mm = O.versa_side_network(tc, tt, P, self.layers[0], self.layers[1], activation=c.act, remove_first=c.rmfirst)
        else:
            cv, text, mm = O.side_network(tc, tt, P, self.layers, activation=c.act, remove_first=c.rmfirst, **self.heads)
        score = F.linear(torch.cat([cv, text, mm], 1), P["com_dense.weight"], P["com_dense.bias"])
        E = score.shape[1]
        prec = O.sasrec(score.view(bs, S + 1, E)[:, :-1], lm, P, 2, 2, drop=drop).reshape(-1, E)
        return O.inbatch_ce(ids, score, prec, lm, pop)


def drop_masks(seed, bs, S, E=64, H=2, L=2, p=0.1):
    """The keep factors of the four SASRec dropout sites of every block for one kernel seed (`O.sasrec`'s `drop`)."""
    masks = {0: helpers.drop_factors(seed, 0, bs * S * E, p).view(bs, S, E)}
    for l in range(L):
        masks[1 + 3 * l] = helpers.drop_factors(seed, 1 + 3 * l, bs * H * S * S, p).view(bs, H, S, S)
        masks[2 + 3 * l] = helpers.drop_factors(seed, 2 + 3 * l, bs * S * E, p).view(bs, S, E)
        masks[3 + 3 * l] = helpers.drop_factors(seed, 3 + 3 * l, bs * S * E, p).view(bs, S, E)
    return masks


def _step_seed(k):
    return 4242 + k


def _kernel_seed(k):
    """The SASRec dropout seed the model draws (`model/modules.py`: one `torch.randint` on the CPU generator per forward) after
    `torch.manual_seed(_step_seed(k))`."""
    torch.manual_seed(_step_seed(k))
    return int(torch.randint(0, 2 ** 62, (1,)).item())


def oracle_trajectory(st: Setup, steps, P0=None, m0=None, v0=None, step0=0, lrs=None, first_batch=0):
    """`steps` Adam steps of the float64 oracle: loss + backward, then `O.adam_step` per tensor with its group's rate."""
    P = {k: v.double().clone() for k, v in (P0 or st.P).items()}
    m = {k: (m0[k].double().clone() if m0 else torch.zeros_like(v)) for k, v in P.items()}
    v = {k: (v0[k].double().clone() if v0 else torch.zeros_like(p)) for k, p in P.items()}
    lrs = lrs or trainer.group_lrs(st.args)
    losses, masks = [], []
    for k in range(first_batch, first_batch + steps):
        b = st.batch(k)
        drop = None
        if st.case.drop > 0:
            drop = drop_masks(_kernel_seed(k), *b.log_mask.shape, p=st.case.drop)
            masks.append(drop)
        Pg = {n: t.clone().requires_grad_(True) for n, t in P.items()}
        loss = st.oracle_loss(Pg, b, drop)
        loss.backward()
        losses.append(loss.item())
        i = step0 + k - first_batch + 1
        for n in P:
            P[n], m[n], v[n] = O.adam_step(P[n], Pg[n].grad, m[n], v[n], i, lrs[O.adam_group_of(n)])
    return dict(P=P, m=m, v=v, losses=losses, masks=masks)


def device_trajectory(st: Setup, tr, steps, first_batch=0, before_step=None):
    losses = []
    for k in range(first_batch, first_batch + steps):
        b = st.batch(k)
        if before_step is not None:
            before_step(tr)
        if st.case.drop > 0:
            torch.manual_seed(_step_seed(k))
        ids, images, text = st.device_inputs(b)
        loss = tr.step(ids, images, text, b.log_mask.cuda())
        losses.append(loss.item())
    torch.cuda.synchronize()
    return losses


def _grouped(names, get):
    """{tensor or gate tower: float64 vector} — the one-scalar gates of a tower held together."""
    out = {}
    for n in names:
        key = n.rsplit(".", 1)[0] if "side_gate" in n else n
        out.setdefault(key, []).append(get(n).reshape(-1).double())
    return {k: torch.cat(v) for k, v in out.items()}


def compare(tr, ref, P0, tag):
    """Worst per-tensor ratios (displacement, m, v) between the trainer's state and the oracle's, and the padding check."""
    params = dict(tr.model.named_parameters())
    off = dict(zip(tr.names, tr.offsets))
    flat, m, v = tr.flat.cpu(), tr.m.cpu(), tr.v.cpu()
    real = torch.zeros(flat.numel(), dtype=torch.bool)
    for n in tr.names:
        real[off[n]:off[n] + params[n].numel()] = True
    for t, what in ((flat, "parameters"), (m, "m"), (v, "v")):
        assert torch.equal(t[~real], torch.zeros(int((~real).sum()))), f"{tag}: alignment padding of the flat {what} is not zero"
    seg = lambda buf: (lambda n: buf[off[n]:off[n] + params[n].numel()])      # noqa: E731
    worst = {}
    for what, got, want, base in (("p", seg(flat), lambda n: ref["P"][n], lambda n: P0[n].double()),
                                  ("m", seg(m), lambda n: ref["m"][n], lambda n: torch.zeros(1, dtype=torch.float64)),
                                  ("v", seg(v), lambda n: ref["v"][n], lambda n: torch.zeros(1, dtype=torch.float64))):
        g = _grouped(tr.names, lambda n: got(n).double() - base(n).reshape(-1))
        r = _grouped(tr.names, lambda n: want(n).reshape(-1) - base(n).reshape(-1))
        ratios = {k: ((g[k] - r[k]).norm() / r[k].norm()).item() for k in g}
        k_w = max(ratios, key=ratios.get)
        worst[what] = (ratios[k_w], k_w)
    return worst


_ORACLE_CACHE = {}


def _oracle_for(name):
    if name not in _ORACLE_CACHE:
        st = Setup(CASES[name])
        _ORACLE_CACHE[name] = oracle_trajectory(st, CASES[name].steps)
    return _ORACLE_CACHE[name]


def run_case(name, before_step=None):
    c = CASES[name]
    st = Setup(c)
    ref = _oracle_for(name)
    tr = trainer.FlatTrainer(st.model, st.args)
    losses = device_trajectory(st, tr, c.steps, before_step=before_step)
    worst = compare(tr, ref, st.P, name)
    dl = max(abs(a - b) / abs(b) for a, b in zip(losses, ref["losses"]))
    return st, tr, ref, losses, worst, dl


@pytest.mark.parametrize("name", list(CASES))
def test_trajectory_matches_float64_oracle(name):
    """K steps of `FlatTrainer.step` (a fresh seeded batch per step, drop_rate 0 except the dropout case) against the same K
    steps of the float64 oracle on the same fp32 tap values: loss at every step, every trainable tensor's displacement and the
    trainer's Adam moments per tensor, the flat buffers' alignment padding exactly zero, and a trajectory that really moves.

    Routes reached: bs 16 the small-M routes and the fused SANB launches (ReLU, and GELU epilogues with layer-0 seeding);
    bs 128 (M = 1,408, the side-net M of the Uncached headline) the `gemm32_dw` / `n64f` / `k64` products; bs 1024 (BASELINE
    config 3) the split-operand `x3` products and the `ce16_*` loss route; Versa the `versa` mode of `sidenet.hip` with a
    dim-align down projection and its Adam group; Uncached the trainer through `IISANAdaptedMModel` and the frozen HIP towers.
    In the Uncached case the oracle is fed the taps the HIP encoders produce for each catalogue item (computed once): tap
    parity is pinned by the encoder tests, and the encoders' fp16 tap error would otherwise dominate the trajectory.  The
    dropout case seeds torch's CPU generator before each step, rebuilds the masks of the counter-based generator on the host
    and passes them to the oracle's SASRec.
    """
    c = CASES[name]
    st, tr, ref, losses, worst, dl = run_case(name)
    print(f"measured: {name}: loss {dl:.2e}, p {worst['p'][0]:.2e} ({worst['p'][1]}), m {worst['m'][0]:.2e} ({worst['m'][1]}), "
          f"v {worst['v'][0]:.2e} ({worst['v'][1]}); oracle loss {ref['losses'][0]:.3f} -> {ref['losses'][-1]:.3f}")
    assert tr.step_no == c.steps
    first, last = ref["losses"][0], float(np.mean(ref["losses"][-3:]))
    assert last < 0.85 * first, f"{name}: trajectory too flat to mean anything ({first:.3f} -> {last:.3f})"
    if c.drop > 0:
        ms = ref["masks"]
        assert all(not torch.equal(ms[i][0], ms[i + 1][0]) for i in range(len(ms) - 1)), "consecutive steps drew the same masks"
    assert dl <= BOUND_LOSS, f"{name}: loss differs by {dl:.2e}"
    assert worst["p"][0] <= BOUND_P, f"{name}: displacement of {worst['p'][1]} off by {worst['p'][0]:.2e}"
    assert worst["m"][0] <= BOUND_MV, f"{name}: m of {worst['m'][1]} off by {worst['m'][0]:.2e}"
    assert worst["v"][0] <= BOUND_MV, f"{name}: v of {worst['v'][1]} off by {worst['v'][0]:.2e}"


# ---------------------------------------------------------------------------------------------------------------
# C.  the comparison rejects a wrong optimiser
# ---------------------------------------------------------------------------------------------------------------

def _zero_moments(tr):
    tr.m.zero_()
    tr.v.zero_()


def _reset_step(tr):
    tr.step_no = 0


def _swap_rates(tr):
    if getattr(tr, "_swapped", False):
        return
    groups = list(dict.fromkeys(trainer.adam_group_of(n) for n in tr.names))
    i, j = groups.index("recsys"), groups.index("adapter_cv")
    tr.seg_lr[i], tr.seg_lr[j] = tr.seg_lr[j], tr.seg_lr[i]
    tr._swapped = True


@pytest.mark.parametrize("broken", ["zero_moments", "reset_step", "swap_rates", "stale_gradient"])
def test_trajectory_comparison_rejects_a_broken_optimiser(broken, monkeypatch):
    """The bs-16 ReLU trajectory rerun with one broken trainer (the breakage lives here, the library is unchanged): the
    metric of `test_trajectory_matches_float64_oracle` must exceed its bound at least tenfold."""
    before = dict(zero_moments=_zero_moments, reset_step=_reset_step, swap_rates=_swap_rates).get(broken)
    if broken == "stale_gradient":                       # the previous step's gradient added back after the backward pass
        real, prev = ops.adam_step, []

        def adam_with_stale_gradient(p, g, *a, **kw):
            cur = g.clone()
            if prev:
                g.add_(prev[0])
            prev[:] = [cur]
            return real(p, g, *a, **kw)
        monkeypatch.setattr(ops, "adam_step", adam_with_stale_gradient)
    name = "cached_relu_bs16"
    _, _, _, _, worst, _ = run_case(name, before_step=before)
    print(f"measured: broken optimiser {broken}: p {worst['p'][0]:.2e} ({worst['p'][1]}) = "
          f"{worst['p'][0] / BOUND_P:.0f}x the bound")
    assert worst["p"][0] >= 10 * BOUND_P, (broken, worst["p"])


# ---------------------------------------------------------------------------------------------------------------
# D.  resuming from a checkpoint written by a stock torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------

def test_resume_from_a_stock_adam_checkpoint_continues_the_oracle_trajectory(tmp_path):
    """K1 steps of the reference's own optimiser (`torch.optim.Adam(build_param_groups(...))`, fed the oracle's gradients
    cast to fp32) on a CPU copy of the model, a checkpoint in the reference's format, `trainer.load_checkpoint` into a device
    model + `FlatTrainer`, then K2 steps on the device against the same K2 steps of the oracle from the same state.  Real
    moments must land on the right one of same-shaped tensors and the bias correction must continue from step K1."""
    K1, K2 = 6, 10
    name = "cached_relu_bs16"
    c = CASES[name]
    st = Setup(c)
    cpu = helpers.build_model(st.args, c.items, st.pop, cached=True, device="cpu")
    helpers.load_trainables(cpu, st.P)
    opt = torch.optim.Adam(trainer.build_param_groups(cpu, st.args))
    named = {n: p for n, p in cpu.named_parameters() if p.requires_grad}
    for k in range(K1):
        Pg = {n: p.detach().double().clone().requires_grad_(True) for n, p in named.items()}
        st.oracle_loss(Pg, st.batch(k)).backward()
        for n, p in named.items():
            p.grad = Pg[n].grad.float()
        opt.step()
    a, b = opt.state[named["mm_encoder.cv_adapter_list.0.fc_down.weight"]], opt.state[named["mm_encoder.cv_adapter_list.1.fc_down.weight"]]
    assert not torch.allclose(a["exp_avg"], b["exp_avg"], rtol=0.1)     # two same-shaped tensors with different moments
    path = str(tmp_path / "resume.pt")
    torch.save({"model_state_dict": {k: v.detach().cpu() for k, v in cpu.state_dict().items()}, "optimizer": opt.state_dict(),
                "rng_state": torch.get_rng_state(), "cuda_rng_state": None}, path)

    tr = trainer.FlatTrainer(st.model, st.args)
    trainer.load_checkpoint(path, st.model, tr)
    assert tr.step_no == K1
    P1 = {n: p.detach().clone() for n, p in named.items()}
    ref = oracle_trajectory(st, K2, P0=P1, m0={n: opt.state[p]["exp_avg"] for n, p in named.items()},
                            v0={n: opt.state[p]["exp_avg_sq"] for n, p in named.items()}, step0=K1, first_batch=K1)
    losses = device_trajectory(st, tr, K2, first_batch=K1)
    assert tr.step_no == K1 + K2
    worst = compare(tr, ref, P1, "resume")
    dl = max(abs(x - y) / abs(y) for x, y in zip(losses, ref["losses"]))
    print(f"measured: resume: loss {dl:.2e}, p {worst['p'][0]:.2e} ({worst['p'][1]}), m {worst['m'][0]:.2e}, v {worst['v'][0]:.2e}")
    assert dl <= BOUND_LOSS, dl
    assert worst["p"][0] <= BOUND_P, worst["p"]
    assert worst["m"][0] <= BOUND_MV and worst["v"][0] <= BOUND_MV, (worst["m"], worst["v"])


# ---------------------------------------------------------------------------------------------------------------
# E.  ranks after training
# ---------------------------------------------------------------------------------------------------------------

def test_ranks_after_training_match_the_oracle_trained_model():
    """After the bs-16 ReLU trajectory: ~200 synthetic users' held-out targets ranked by the HIP eval path
    (`evaluate.item_table`, `evaluate.evaluate_ranks`) on the device-trained model, and by the oracle (`O.side_network` over
    the catalogue, `O.sasrec` at the last position, `O.eval_ranks`) on the oracle-trained parameters."""
    name = "cached_relu_bs16"
    st, tr, ref, _, _, _ = run_case(name)
    U, S = 200, st.args.max_seq_len
    ids, _ = synth.make_ids(U, S, st.case.items, np.random.RandomState(77))
    seqs = [[int(x) for x in row if x != 0] for row in ids]
    hists = [s[:-1] for s in seqs]
    tc, tt = st.tabs[0].cuda(), st.tabs[1].cuda()
    emb = evaluate.item_table(st.model, tc, tt)
    got = evaluate.evaluate_ranks(st.model, emb, seqs, hists, S).cpu().to(torch.int64)

    P = ref["P"]
    with torch.no_grad():
        cv, text, mm = O.side_network(st.tabs[0].double(), st.tabs[1].double(), P, st.layers, activation=st.case.act, **st.heads)
        emb_o = F.linear(torch.cat([cv, text, mm], 1), P["com_dense.weight"], P["com_dense.bias"])
        tok = torch.zeros(U, S, dtype=torch.int64)
        lm = torch.zeros(U, S, dtype=torch.float64)
        for u, s in enumerate(seqs):
            h = s[:-1][-S:]
            tok[u, S - len(h):] = torch.tensor(h)
            lm[u, S - len(h):] = 1
        prec = O.sasrec(emb_o[tok], lm, P, 2, 2)[:, -1]
        want = O.eval_ranks(prec, emb_o, [torch.tensor(h, dtype=torch.int64) for h in hists],
                            torch.tensor([s[-1] for s in seqs]))
    same = (got == want).double().mean().item()
    dmax = (got - want).abs().max().item()
    h_got, n_got = O.hit_ndcg(got)
    h_want, n_want = O.hit_ndcg(want)
    dh, dn = abs(h_got.mean() - h_want.mean()).item(), abs(n_got.mean() - n_want.mean()).item()
    print(f"measured: ranks after training: {same:.3f} equal, max |diff| {dmax}, Hit@10 {h_got.mean():.4f} vs "
          f"{h_want.mean():.4f}, nDCG@10 {n_got.mean():.4f} vs {n_want.mean():.4f}")
    assert same >= 0.98, same              # measured on MI355X: 199 of 200 users equal, the other one rank apart
    assert dmax <= 2, dmax
    assert dh <= (1 - same) + 1e-9 and dn <= (1 - same) + 1e-9, (dh, dn)
