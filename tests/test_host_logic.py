"""CPU tests of the host-side logic: module tree / state-dict keys, freeze + Adam-group rules, parameter tables of the
C ABI, flat trainer storage, synthetic batches, HF <-> canonical weight conversion."""
import json
import os

import numpy as np
import pytest
import torch

import golden_io as gio
import helpers
from iisan_amd import ops, synth, trainer, weights


def _tiny_cfgs():
    return (weights.VitConfig(hidden=768, layers=1, heads=12, mlp=128, image=32, patch=16),
            weights.BertConfig(hidden=768, layers=1, heads=12, mlp=128, vocab=64, max_pos=16))


def test_uncached_module_tree_has_the_reference_trainable_names():
    args = helpers.make_args()
    model = helpers.build_model(args, 100, torch.ones(101), cached=False, device="cpu")
    names = {n for n, p in model.named_parameters() if p.requires_grad}
    want = set(weights.trainable_shapes())
    assert names == want, names ^ want
    shapes = weights.trainable_shapes()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert tuple(p.shape) == shapes[n], n
    assert sum(p.numel() for p in model.parameters() if p.requires_grad) == 4113877


def test_cached_module_tree_names():
    args = helpers.make_args()
    model = helpers.build_model(args, 100, torch.ones(101), cached=True, device="cpu")
    names = {n for n, p in model.named_parameters() if p.requires_grad}
    assert names == set(weights.trainable_shapes(cached=True))


def test_adam_groups_follow_reference_rule():
    groups = json.load(open(os.path.join(gio.GOLDEN, "adam_groups.json")))
    for n, g in groups.items():
        assert trainer.adam_group_of(n) == g, n
    args = helpers.make_args()
    model = helpers.build_model(args, 100, torch.ones(101), cached=False, device="cpu")
    pg = trainer.build_param_groups(model, args)
    assert [len(g["params"]) for g in pg] == [2, 9, 51, 56, 28]          # text_encoder, image_net, recsys, adapter_cv, adapter_text
    assert [g["lr"] for g in pg] == [5e-5, 1e-4, 2e-4, 1e-4, 1e-4]


def test_abi_parameter_tables_resolve():
    args = helpers.make_args()
    for cached in (False, True):
        model = helpers.build_model(args, 100, torch.ones(101), cached=cached, device="cpu")
        side = dict(model.mm_encoder.named_parameters())
        order = ops.side_param_order(7, cached)
        assert len(order) == 15 * 7 + 12 and all(k in side for k in order)
    te = dict(model.user_encoder.transformer_encoder.named_parameters())
    order = ops.sasrec_param_order(2)
    assert len(order) == 27 and set(order) == set(te)


@pytest.mark.parametrize("cached", [False, True])
def test_unequal_adapter_widths_are_refused_at_construction(cached):
    """The reference builds the cv adapters with `cv_adapter_down_size` and the text / mm adapters with `bert_adapter_down_size`
    (`model.py:178-189`); `iisan_side_cfg` has ONE `down`, so a model with two widths would hand the kernels `[16, 768]` tensors
    they index as `[64, 768]`.  Both IISAN wrappers refuse it like the Versa wrapper does; equal widths of any value build."""
    args = helpers.make_args(cv_adapter_down_size=16, bert_adapter_down_size=64)
    with pytest.raises(NotImplementedError, match="one bottleneck width for all towers"):
        helpers.build_model(args, 100, torch.ones(101), cached=cached, device="cpu")
    model = helpers.build_model(helpers.make_args(cv_adapter_down_size=16, bert_adapter_down_size=16), 100, torch.ones(101),
                                cached=cached, device="cpu")
    assert model.mm_encoder.cv_adapter_list[0].fc_down.out_features == 16


def _iisan_side_cfg(enc, n_taps=13):
    """The `iisan_side_cfg` `_SideNetBase._side` builds for taps [M, n_taps, 768] (Cached: the layer list indexes the tap axis)."""
    return ops.make_side_cfg(enc.n_side, 768, enc.mm_adapter_list[0].fc_down.out_features, enc.fc_mm_down.out_features, enc.gated,
                             enc.mm_adapter_list[0].gelu, enc.remove_first, n_taps, n_taps, list(enc.side_cv_adapter_num_list), 0)


@pytest.mark.parametrize("kw", [dict(), dict(remove_first="TRUE"), dict(cv_adapter_down_size=32, bert_adapter_down_size=32),
                                dict(fusion_method="sum"), dict(modality="inter")], ids=["default", "rmfirst", "down32", "sum", "inter"])
@pytest.mark.parametrize("cached", [False, True])
def test_side_param_shapes_equal_the_module_tree(kw, cached):
    """`ops.side_param_shapes(cfg)` - what `SideNetFn` holds every tensor to before a launch - is the shape of every tensor the
    wrapper hands over, in ABI order, placeholders (absent gates / towers) included."""
    model = helpers.build_model(helpers.make_args(**kw), 100, torch.ones(101), cached=cached, device="cpu")
    enc = model.mm_encoder
    got = [tuple(t.shape) for t in enc._abi_params(torch.device("cpu"))]
    want = ops.side_param_shapes(_iisan_side_cfg(enc))
    assert len(want) == 15 * enc.n_side + 12
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4]
    r = 32 if "cv_adapter_down_size" in kw else 64
    assert want[0] == (r, 768) and want[2] == (768, r) and want[12 * enc.n_side] == (1,) and want[-2] == (64, 768)


@pytest.mark.parametrize("variant", sorted(gio.VERSA_VARIANTS))
def test_side_param_shapes_equal_the_versa_module_tree(variant):
    """The same for the Versa wrapper: towers of different depth and width, the dim-align pairs where the widths differ."""
    Di, Dt, Lc, Lt, vlist, blist, extra = gio.VERSA_VARIANTS[variant]
    args = helpers.make_args(text_embedding_dim=Dt, image_embedding_dim=Di, side_adapter_vit_list=vlist, side_adapter_bert_list=blist,
                             image_layers=Lc - 1, text_layers=Lt - 1, **extra)
    enc = helpers.build_model(args, 50, torch.ones(51), cached="versa", device="cpu").mm_encoder
    cfg = ops.make_versa_cfg(Di, Dt, args.cv_adapter_down_size, args.embedding_dim, enc.gated, args.adapter_activation == "GELU",
                             enc.remove_first, Lc, Lt, enc.side_cv_adapter_num_list, enc.side_bert_adapter_num_list)
    got = [tuple(t.shape) for t in enc._abi_params(torch.device("cpu"))]
    want = ops.side_param_shapes(cfg)
    n_mm = min(enc.n_cv, enc.n_t)
    assert len(want) == 5 * (enc.n_cv + enc.n_t + n_mm) + (2 * n_mm if Di != Dt else 0) + 12
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4]


def test_mis_shaped_parameter_tables_are_named_before_anything_runs():
    """`ops._check_shapes` (the comparison `SideNetFn.forward` / `SasrecFn.forward` make before the workspace query): the first
    offending slot is named with both shapes; the SASRec position table may be longer than `seq`, never shorter or narrower."""
    from iisan_amd import _lib
    model = helpers.build_model(helpers.make_args(), 100, torch.ones(101), cached=True, device="cpu")
    enc = model.mm_encoder
    cfg = _iisan_side_cfg(enc)
    params = enc._abi_params(torch.device("cpu"))
    ops._check_shapes("side network", ops._side_param_slots(cfg), params)
    bad = list(params)
    bad[4] = torch.zeros(16, 768)                               # cv_adapter_list.1.fc_down.weight
    with pytest.raises(_lib.IisanHipError, match=r"slot 4 \(cv_adapter_list.1.fc_down.weight\) has shape \(16, 768\).*\(64, 768\)"):
        ops._check_shapes("side network", ops._side_param_slots(cfg), bad)
    with pytest.raises(_lib.IisanHipError, match="expects 117 parameter tensors, got 116"):
        ops._check_shapes("side network", ops._side_param_slots(cfg), params[:-1])
    te = model.user_encoder.transformer_encoder
    sp = te.abi_params()
    for seq in (10, 7):                                         # a window shorter than the table is served
        ops._check_shapes("sasrec", ops._sasrec_param_slots(ops.make_sasrec_cfg(seq, 64, 2, 2)), sp)
    with pytest.raises(_lib.IisanHipError, match=r"slot 0 \(position_embedding.weight\) has shape \(10, 64\).*\(>= 11, 64\)"):
        ops._check_shapes("sasrec", ops._sasrec_param_slots(ops.make_sasrec_cfg(11, 64, 2, 2)), sp)
    with pytest.raises(_lib.IisanHipError, match=r"w_1.weight\) has shape \(256, 64\).*\(512, 128\)"):
        ops._check_shapes("sasrec", ops._sasrec_param_slots(ops.make_sasrec_cfg(10, 128, 2, 2)), [torch.zeros(10, 128)] + [torch.zeros(128)] * 2
                          + [torch.zeros(128, 128)] * 4 + [torch.zeros(128)] * 2 + sp[9:])


def test_flat_trainer_storage_is_contiguous_by_group():
    args = helpers.make_args()
    model = helpers.build_model(args, 100, torch.ones(101), cached=True, device="cpu")
    before = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    tr = trainer.FlatTrainer(model, args)
    assert tr.n_params == 4113877 and tr.seg_end[-1] == tr.flat.numel() and len(tr.seg_end) == 5
    assert all(o % 16 == 0 for o in tr.offsets) and tr.flat.numel() - tr.n_params < 16 * len(tr.names)
    assert tr.seg_lr == [5e-5, 1e-4, 2e-4, 1e-4, 1e-4]
    base = tr.flat.data_ptr()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert torch.equal(p.detach(), before[n])
            off = (p.data_ptr() - base) // 4
            assert 0 <= off < tr.flat.numel() and p.grad.data_ptr() - tr.grad.data_ptr() == p.data_ptr() - base
    g = sorted((trainer.GROUP_ORDER.index(trainer.adam_group_of(n)), (dict(model.named_parameters())[n].data_ptr() - base) // 4)
               for n in tr.names)
    assert [o for _, o in g] == sorted(o for _, o in g)            # group index is monotone in the flat offset


def test_synthetic_batch_contract():
    b = synth.scientific_batch(bs=16, seed=1, res=32)
    assert b.ids.shape == (16, 11) and b.log_mask.shape == (16, 10) and b.images.shape == (176, 3, 32, 32)
    assert b.text.shape == (176, 60) and b.pop_prob[0] == 1 and (b.pop_prob > 0).all()
    ids = b.ids.numpy()
    for r in ids:                                                   # left padded, >= 2 real items, unique within a row
        nz = r[r != 0]
        assert len(nz) >= 2 and (r[:11 - len(nz)] == 0).all() and len(set(nz)) == len(nz)
    assert torch.equal(b.log_mask, (b.ids[:, :-1] != 0).float())
    pad = (b.ids.view(-1) == 0)
    assert (b.images[pad] == 0).all() and (b.text[pad] == 0).all()
    assert (b.text[~pad][:, 0] == 101).all() and (b.text[~pad][:, 30] == 1).all()
    assert b.images.abs().max() <= 1.0


def test_hf_weight_roundtrip():
    vcfg, bcfg = _tiny_cfgs()
    vw, bw = weights.make_vit_weights(vcfg, 1), weights.make_bert_weights(bcfg, 2)
    back = weights.vit_from_hf(weights.vit_to_hf5(vw, vcfg))
    assert set(back) == set(vw) and all(torch.equal(back[k], vw[k]) for k in vw)
    back = weights.bert_from_hf(weights.bert_to_hf(bw, bcfg))
    assert set(back) == set(bw) and all(torch.equal(back[k], bw[k]) for k in bw)
    # 4.x layout of the same ViT weights
    sd5 = weights.vit_to_hf5(vw, vcfg)
    sd4 = {}
    for k, v in sd5.items():
        k = k.replace("vit.layers.", "vit.encoder.layer.").replace("attention.q_proj", "attention.attention.query") \
             .replace("attention.k_proj", "attention.attention.key").replace("attention.v_proj", "attention.attention.value") \
             .replace("attention.o_proj", "attention.output.dense").replace("mlp.fc1", "intermediate.dense").replace("mlp.fc2", "output.dense")
        sd4[k] = v
    back4 = weights.vit_from_hf(sd4)
    assert all(torch.equal(back4[k], vw[k]) for k in vw)


def test_oracle_invariants_padding_has_zero_influence():
    """padding slots contribute exactly nothing to the loss."""
    from oracle import iisan_oracle as O
    z, b, taps_cv, taps_tx, P, kw = gio.sidenet_full_inputs("default")
    layers = O.side_layer_list("1,3,5,7,9,11", False)
    kwargs = dict(cv_head="mm_encoder.cv_pre_fc.", text_head="mm_encoder.bert_pre_fc.")
    l0, _ = O.model_loss_from_taps(b.ids, taps_cv, taps_tx, b.log_mask, b.pop_prob, P, layers, **kwargs)
    pad = (b.ids.view(-1) == 0)
    tc, tt = taps_cv.clone(), taps_tx.clone()
    tc[pad] = torch.randn_like(tc[pad]) * 3
    tt[pad] = torch.randn_like(tt[pad]) * 3
    l1, _ = O.model_loss_from_taps(b.ids, tc, tt, b.log_mask, b.pop_prob, P, layers, **kwargs)
    assert torch.equal(l0, l1)


def test_checkpoint_format_matches_torch_adam_and_round_trips(tmp_path):
    """checkpoints carry the reference's keys (utils.py:104-110) and the optimizer entry is a genuine
    torch.optim.Adam state dict over run.py's five groups — loadable by a stock Adam — and round-trips."""
    import helpers
    from iisan_amd import synth, trainer
    args = helpers.make_args()
    model = helpers.build_model(args, 30, synth.make_pop_prob(30), cached=True, device="cpu")     # wired + frozen like run.py
    tr = trainer.FlatTrainer(model, args)
    g = torch.Generator().manual_seed(3)
    real = torch.zeros(tr.flat.numel(), dtype=torch.bool)        # the alignment padding between tensors holds no state
    for (_, o, k, _) in trainer._segments(tr):
        real[o:o + k] = True
    tr.m.copy_(torch.rand(tr.m.shape, generator=g) * real)
    tr.v.copy_(torch.rand(tr.v.shape, generator=g) * real)
    tr.step_no = 7
    before = tr.flat.clone()
    sd = trainer.optimizer_state_dict(tr)
    ref_opt = torch.optim.Adam(trainer.build_param_groups(model, args))
    ref_sd = ref_opt.state_dict()
    assert [len(g_["params"]) for g_ in sd["param_groups"]] == [len(g_["params"]) for g_ in ref_sd["param_groups"]] == [2, 9, 51, 56, 28]
    assert [g_["lr"] for g_ in sd["param_groups"]] == [g_["lr"] for g_ in ref_sd["param_groups"]]
    ref_opt.load_state_dict(sd)                                  # a stock optimiser accepts it ...
    flat_params = [p for g_ in ref_opt.param_groups for p in g_["params"]]
    for i, p in enumerate(flat_params):                          # ... and lands every moment on the right tensor
        st = ref_opt.state[p]
        assert st["exp_avg"].shape == p.shape and float(st["step"]) == 7.0
    path = str(tmp_path / "epoch-3.pt")
    trainer.save_checkpoint(path, model, tr)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"model_state_dict", "optimizer", "rng_state", "cuda_rng_state"}
    m0, v0 = tr.m.clone(), tr.v.clone()
    tr.m.zero_(); tr.v.zero_(); tr.step_no = 0
    with torch.no_grad():
        for p in model.parameters():                             # (the alignment padding of the flat buffer stays zero)
            if p.requires_grad:
                p.add_(1.0)
    trainer.load_checkpoint(path, model, tr)
    assert torch.equal(tr.flat, before) and torch.equal(tr.m, m0) and torch.equal(tr.v, v0) and tr.step_no == 7
    for n, p in model.named_parameters():                        # still views of the flat buffer
        if p.requires_grad:
            assert p.data.untyped_storage().data_ptr() == tr.flat.untyped_storage().data_ptr(), n


def test_real_huggingface_modules_are_accepted_at_the_boundary():
    """The drop-in boundary as `Code_Uncached/run.py:50-100,161` uses it: a `ViTForImageClassification` (classifier
    re-created as Linear(768, 64), run.py:56-61) and a `BertModel(output_hidden_states=True)` built from the values of the
    reference's `pretrained_models/*/config.json` go straight into the product `ModelMM`.  The weight extraction the HIP
    encoders pack from (`model/encoders.py:_vit_canonical/_bert_canonical`) must return exactly the weights that were
    loaded — for the installed transformers' key layout (5.x: `vit.layers.N.attention.q_proj`) and for the reference's
    pinned 4.20.1 layout (`vit.encoder.layer.N.attention.attention.query`)."""
    import pytest
    tf = pytest.importorskip("transformers")
    from torch import nn
    from iisan_amd.model import ModelMM
    from iisan_amd.model.encoders import _bert_canonical, _vit_canonical
    vcfg, bcfg = weights.VIT_BASE, weights.BERT_BASE
    vw, bw = weights.make_vit_weights(), weights.make_bert_weights()
    hf_v = tf.ViTConfig(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, image_size=224,
                        patch_size=16, num_channels=3, qkv_bias=True, layer_norm_eps=1e-12, hidden_act="gelu",
                        hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf_b = tf.BertConfig(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                         vocab_size=30522, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                         hidden_act="gelu", output_hidden_states=True)
    vit = tf.ViTForImageClassification(hf_v)
    missing, unexpected = vit.load_state_dict(weights.vit_to_hf5(vw, vcfg), strict=False)
    assert not unexpected and all(k.startswith("classifier") for k in missing), (missing, unexpected)
    vit.classifier = nn.Linear(vit.classifier.in_features, 64)                       # run.py:59-60
    bert = tf.BertModel(hf_b)
    missing, unexpected = bert.load_state_dict(weights.bert_to_hf(bw, bcfg), strict=False)
    assert not unexpected and all("pooler" in k or "position_ids" in k for k in missing), (missing, unexpected)

    args = helpers.make_args()
    model = ModelMM(args, 100, True, vit, bert, torch.ones(101))
    trainer.apply_iisan_freeze_rules(model, args, cached=False)
    # same trainable set and sizes as with the light containers — and as the reference (199,394,773
    # parameters of which 4,113,877 trainable; the pooler is there and frozen, run.py:83-100)
    names = {n for n, p in model.named_parameters() if p.requires_grad}
    assert names == set(weights.trainable_shapes())
    assert sum(p.numel() for p in model.parameters() if p.requires_grad) == 4113877
    assert sum(p.numel() for p in model.parameters()) == 199394773
    assert "mm_encoder.cv_encoder.image_net.vit.embeddings.cls_token" in model.state_dict()
    assert "mm_encoder.bert_encoder.text_encoders.title.bert_model.embeddings.word_embeddings.weight" in model.state_dict()

    gv, gcfg = _vit_canonical(model.mm_encoder.cv_encoder.image_net)
    assert gcfg == vcfg and set(gv) == set(vw) and all(torch.equal(gv[k], vw[k]) for k in vw)
    gb, gbcfg = _bert_canonical(model.mm_encoder.bert_encoder.text_encoders["title"].bert_model)
    assert gbcfg == bcfg and set(gb) == set(bw) and all(torch.equal(gb[k], bw[k]) for k in bw)

    class Vit4x(nn.Module):                       # the same module as transformers 4.20.1 names its tensors
        def __init__(self, inner):
            super().__init__()
            self.inner, self.config = inner, inner.config

        def state_dict(self, *a, **k):
            ren = (("vit.layers.", "vit.encoder.layer."), ("attention.q_proj", "attention.attention.query"),
                   ("attention.k_proj", "attention.attention.key"), ("attention.v_proj", "attention.attention.value"),
                   ("attention.o_proj", "attention.output.dense"), ("mlp.fc1", "intermediate.dense"), ("mlp.fc2", "output.dense"))
            out = {}
            for key, v in self.inner.state_dict().items():
                for a_, b_ in ren:
                    key = key.replace(a_, b_)
                out[key] = v
            return out

    is5 = any(k.startswith("vit.layers.") for k in vit.state_dict())
    g4, _ = _vit_canonical(Vit4x(vit) if is5 else vit)
    assert any(".encoder.layer." in k for k in (Vit4x(vit) if is5 else vit).state_dict())
    assert all(torch.equal(g4[k], vw[k]) for k in vw)


def test_bench_starts_its_own_ranks_and_describes_the_host():
    """`python bench.py --gpus N` outside a rank environment must launch N fresh ranks itself (it used to
    exit non-zero), with the rendezvous on 127.0.0.1 and its own arguments passed through."""
    import importlib.util
    import sys
    import pytest
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(gio.GOLDEN.rstrip("/")), "..", "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    a = bench.parse(["--gpus", "8", "--steps", "4", "--warmup", "1"])
    cmd = bench.launch_command(a, ["--gpus", "8", "--steps", "4", "--warmup", "1"], 29123)
    assert cmd[0] == sys.executable and cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29123"
    i = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "8", "--steps", "4", "--warmup", "1"]
    assert bench.parse([]).bs == 128 and bench.parse(["--cached", "fp32"]).bs == 1024 and bench.parse(["--cached", "fp16", "--versa"]).bs == 128
    assert not bench.parse([]).full and bench.parse(["--full"]).full and bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"
    for other in (["--eval"], ["--cached", "fp32"]):          # --dump-outputs writes the headline path's outputs only
        with pytest.raises(SystemExit):
            bench.parse(["--dump-outputs", "d"] + other)
    cores, model = bench.host_cpu()
    assert 1 <= cores <= (os.cpu_count() or 1) and isinstance(model, str) and model


def test_hit_ndcg_never_counts_the_invalid_target_signal_as_a_hit():
    """`iisan_score_rank` answers -1 for a target outside 1..item_num (the reference raises IndexError, metrics.py:206);
    `hit_ndcg` must not read that as rank <= 10."""
    from iisan_amd import evaluate
    hit, ndcg = evaluate.hit_ndcg(torch.tensor([1, 3, 11, -1]))
    assert abs(hit - 2 / 4) < 1e-12
    assert abs(ndcg - (1.0 + 0.5) / 4) < 1e-12


def test_bench_refuses_an_rccl_line_with_two_ranks_on_one_device():
    """the first 8-GPU SCALE run must verify itself — a multi-rank line under backend nccl whose ranks do
    not each own a device is refused (gloo with both ranks on cuda:0 is the single-GPU test transport and passes)."""
    import importlib.util
    import pytest
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(os.path.dirname(gio.GOLDEN.rstrip("/")), "..", "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    r = lambda dev, uuid, host="n0": {"rank": dev, "host": host, "device": dev, "uuid": uuid}
    bench.check_one_device_per_rank("nccl", [r(0, "GPU-a"), r(1, "GPU-b")])
    bench.check_one_device_per_rank("nccl", [r(0, ""), r(1, "")])                      # no uuid reported: device indices differ
    bench.check_one_device_per_rank("nccl", [r(0, "00000000"), r(1, "00000000")])      # a runtime with degenerate uuids
    bench.check_one_device_per_rank("nccl", [r(0, "GPU-a", "n0"), r(0, "GPU-a", "n1")])  # same index on two hosts
    bench.check_one_device_per_rank("gloo", [r(0, "GPU-a"), r(0, "GPU-a")])
    with pytest.raises(SystemExit):
        bench.check_one_device_per_rank("nccl", [r(0, "GPU-a"), r(0, "GPU-a")])
    with pytest.raises(SystemExit):
        bench.check_one_device_per_rank("nccl", [r(0, ""), r(0, "")])


def test_h256_head_major_addressing_bound_is_independent_of_which0():
    """`gemm16_h256_kernel` stores head-major QKV through 32-bit byte offsets into [item][head][3][S][64]; the
    element-row index reaches rows * 3 * heads whatever `qkv_which0` is, so the applicability bound must too (it used 3 - which0:
    row counts in [932k, 1.40M) passed with which0 = 1 and the offsets wrapped).  Pure host logic: no device is touched."""
    from iisan_amd import _lib
    lib = _lib.load()
    QKV = 4                                       # EPI_QKVH16
    heads, S = 12, 197
    limit = (1 << 32) // (3 * heads * 128)        # rows beyond this cannot be addressed with 32 bits
    for which0, N in ((0, 2304), (1, 1536)):
        assert lib.iisan_gemm16_h256_applicable(QKV, 277376, N, 768, S, heads, which0) == 1          # the production shape
        assert lib.iisan_gemm16_h256_applicable(QKV, 256 * (limit // 256 - 1), N, 768, S, heads, which0) == 1
        for rows in (940_000, 1_200_000, 1_390_000, 256 * (limit // 256 + 1)):
            assert lib.iisan_gemm16_h256_applicable(QKV, rows, N, 768, S, heads, which0) == 0, (which0, rows)
    # the 16-bit row-major epilogues keep their own (leading-dimension) bound
    assert lib.iisan_gemm16_h256_applicable(0, 1_390_000, 768, 768, 0, 0, 0) == 1
    assert lib.iisan_gemm16_h256_applicable(0, 277376, 768, 64, 0, 0, 0) == 0                       # K / 64 < 2


def test_gemm16_route_table_under_every_variant():
    """The kernel family `launch_gemm16` gives a product (gemm16.hip: gemm16_route, the ONE place that decides), as a literal table:
    2 = gemm16_h256, 1 = gemm16_s256, 0 = the 128x128 kernel, -1 = rejected, under gemm16_variant 0..4.  With T = ceil(M/256) * (N/256):
    variant 0 takes h256, else s256, where T >= 128 and the kernel is applicable; 1 and 2 force 128x128; 3 forces s256 and 4 forces h256
    where applicable; LayerNorm row statistics (+ln) and the stream epilogue exist on h256 with fp16 operands only.  A changed threshold
    fails here, on a CPU, and not only in the GPU counter test of the bench shapes.  Pure host logic: no device is touched."""
    from iisan_amd import _lib
    lib = _lib.load()
    F16, BF16 = 0, 1
    OUT16, GELU16, RESID32, QKVH16, PATCH16, STREAM16 = 0, 1, 2, 4, 6, 7
    M = 277_376                                   # bs = 128 headline batch: 1,408 images x 197 tokens
    # (dtype, mode, M, N, K, S (P for PATCH16), heads, which0, +ln) -> route under variants 0..4
    table = [
        ((F16, QKVH16, M, 2304, 768, 197, 12, 0, 0), (2, 0, 0, 1, 2)),
        ((F16, QKVH16, M, 2304, 768, 197, 12, 0, 1), (2, -1, -1, -1, 2)),
        ((F16, QKVH16, M, 1536, 768, 197, 12, 1, 1), (2, -1, -1, -1, 2)),          # K / V only (CLS-pruned last block)
        ((F16, GELU16, M, 3072, 768, 0, 0, 0, 0), (2, 0, 0, 1, 2)),
        ((F16, GELU16, M, 3072, 768, 0, 0, 0, 1), (2, -1, -1, -1, 2)),
        ((F16, STREAM16, M, 768, 768, 197, 0, 0, 0), (2, -1, -1, -1, 2)),
        ((F16, STREAM16, M, 768, 3072, 197, 0, 0, 0), (2, -1, -1, -1, 2)),
        ((F16, OUT16, M, 768, 768, 0, 0, 0, 0), (2, 0, 0, 1, 2)),
        ((F16, OUT16, M, 768, 3072, 0, 0, 0, 0), (2, 0, 0, 1, 2)),
        ((F16, PATCH16, 275_968, 768, 768, 196, 0, 0, 0), (2, 0, 0, 0, 2)),        # gemm16_s256 has no patch epilogue
        ((F16, OUT16, 1_408, 768, 768, 0, 0, 0, 0), (0, 0, 0, 1, 2)),              # T = 18 < 128: auto stays on 128x128
        ((F16, OUT16, M, 768, 64, 0, 0, 0, 0), (0, 0, 0, 0, 0)),                   # K / 64 < 2: no 256x256 kernel
        ((F16, RESID32, M, 768, 768, 0, 0, 0, 0), (0, 0, 0, 0, 0)),                # fp32 epilogues: 128x128 only
        ((F16, STREAM16, 1_408, 768, 768, 197, 0, 0, 0), (-1, -1, -1, -1, 2)),
        ((BF16, STREAM16, M, 768, 768, 197, 0, 0, 0), (-1, -1, -1, -1, -1)),
        ((BF16, QKVH16, M, 2304, 768, 197, 12, 0, 1), (-1, -1, -1, -1, -1)),
        ((BF16, QKVH16, M, 2304, 768, 197, 12, 0, 0), (2, 0, 0, 1, 2)),
        ((F16, OUT16, M, 768, 768, 0, 0, 0, 1), (-1, -1, -1, -1, -1)),             # +ln: QKV and FC1 products only
        ((F16, GELU16, M, 8192, 768, 0, 0, 0, 1), (-1, -1, -1, -1, -1)),           # +ln: N <= 6144
        ((F16, GELU16, M, 8192, 768, 0, 0, 0, 0), (2, 0, 0, 1, 2)),
        ((F16, GELU16, M, 16384, 768, 0, 0, 0, 0), (0, 0, 0, 0, 0)),               # wider than the bias slot of either 256x256 kernel
        # the size rule at its boundary (N / 256 = 4): 31 row tiles -> T = 124, one row more -> 32 row tiles, T = 128
        ((F16, OUT16, 7_936, 1024, 768, 0, 0, 0, 0), (0, 0, 0, 1, 2)),
        ((F16, OUT16, 7_937, 1024, 768, 0, 0, 0, 0), (2, 0, 0, 1, 2)),
        # beyond the 32-bit addressing bound of gemm16_h256's head-major store (the test above): auto falls to s256, variant 4 never does
        ((F16, QKVH16, 1_200_000, 2304, 768, 197, 12, 0, 0), (1, 0, 0, 1, 0)),
        # the shape checks launch_gemm16 makes up front count as rejected
        ((F16, OUT16, M, 832, 768, 0, 0, 0, 0), (-1, -1, -1, -1, -1)),             # N % 128
        ((F16, OUT16, M, 768, 800, 0, 0, 0, 0), (-1, -1, -1, -1, -1)),             # K % 64
        ((F16, QKVH16, M, 2304, 768, 197, 8, 0, 0), (-1, -1, -1, -1, -1)),         # N != 3 * 64 * heads
        ((F16, PATCH16, 275_968, 768, 768, 0, 0, 0, 0), (-1, -1, -1, -1, -1)),     # patch mode needs P
    ]
    for variant in range(5):
        with _lib.dev(gemm16_variant=variant):
            for args, want in table:
                got = lib.iisan_gemm16_route(*args)
                assert (got if got >= 0 else -1) == want[variant], (variant, args, got, want[variant])


def test_inbatch_ce_route_table_under_every_ce_fast():
    """The route of one loss call (ce.hip: ce_route, the ONE place that decides; the forward call's token carries it to the backward call),
    as a literal table under ce_fast 0..4: G = generic kernel, R = separate row passes, F = fused f32 row pass, X = split-operand passes.
    The row-fixed kernels take 5 <= S <= 15; the default (1) goes to the split-operand route from 2^24 logits on; shapes `check()` rejects
    are negative.  Pure host logic: no device is touched."""
    from iisan_amd import _lib
    lib = _lib.load()
    G, R, F, X = 0, 1, 2, 3
    table = [
        ((3, 10), (G, F, R, X, F)),
        ((128, 10), (G, F, R, X, F)),
        ((64, 15), (G, F, R, X, F)),                 # RS1 = 16
        ((1024, 10), (G, X, R, X, F)),
        ((390, 10), (G, F, R, X, F)),                # 390^2 * 110 = 16,731,000 < 2^24
        ((391, 10), (G, X, R, X, F)),                # 391^2 * 110 = 16,816,910 >= 2^24
        ((64, 4), (G, G, G, G, G)),                  # S too small: a 16-row tile would span more than four sequences
        ((64, 16), (G, G, G, G, G)),                 # S + 1 > 16 ids per sequence
        ((0, 10), None),
        ((64, 64), None),
    ]
    for ce_fast in range(5):
        with _lib.dev(ce_fast=ce_fast):
            for (bs, S), want in table:
                got = lib.iisan_inbatch_ce_route(bs, S)
                if want is None:
                    assert got < 0, (ce_fast, bs, S, got)
                else:
                    assert got == want[ce_fast], (ce_fast, bs, S, got, want[ce_fast])


def test_gemm32_plan_table():
    """What `launch_gemm32` does with a group of fp32 products (gemm32.hip: plan_gemm32, decided before anything is launched), as a literal
    table.  THE PLAN DEPENDS ON `iisan_cu_count`: the weight-gradient split counts below are those of 256 compute units — an MI355X, and the
    value the library assumes where no device is visible, so the table holds on a CPU.  Expected values: recorded from the launcher this
    plan replaced (its decisions at each launch, on the same inputs), which agreed with every hand-derived anchor (#1 - #8: the side
    network's launches at the bench shapes).  Fields: kernel (0 tiled, 1 K = 64, 2 weight-gradient, 3 split into a K = 64 launch and a rest
    launch), row-tile height, K splits, scratch (0 none, 1 partials + epilogue reducer, 2 partials added to C), fast fetch, three K-tiles in
    flight, column sums (0 none, 1 out of the product, 2 own launch), column blocks (K = 64 kernel), grid x / y / z, K = 64 members of a split."""
    import ctypes as C
    from iisan_amd import _lib
    lib = _lib.load()
    TA, TB, RELU, GELU, ACCUM, MASK, PREACT = 1, 2, 4, 8, 16, 32, 128
    DW = TA | TB | ACCUM
    AMPLE = 1 << 28
    cached6 = [(768, 64, 11264)] * 3 + [(64, 768, 11264)] * 3      # dWu and dWd of a Cached SANB step (bs = 1024), three towers
    versa6 = [(1024, 64, 1408), (8192, 64, 1408), (1024, 64, 1408), (64, 1024, 1408), (64, 8192, 1408), (64, 1024, 1408)]
    k64 = [(11264, 768, 64)] * 3
    # (problems (M, N, K), flags, scratch floats, with column sums, dev switches) -> plan
    table = [
        (cached6, DW, AMPLE, 1, {}, (2, 64, 7, 2, 0, 0, 1, 0, 12, 7, 6, 0)),                        # 1: 72 tiles x 7 = two workgroups per CU
        (cached6[:3], DW, AMPLE, 1, {}, (2, 64, 7, 2, 0, 0, 1, 0, 12, 7, 3, 0)),                    # 2: 36 tiles x 7 = one per CU
        (versa6, DW, AMPLE, 1, {}, (2, 64, 2, 2, 0, 0, 1, 0, 128, 2, 6, 0)),                        # 3
        (k64, 0, AMPLE, 0, {}, (1, 0, 0, 0, 0, 0, 0, 4, 176, 3, 3, 0)),                             # 4: up projection + residual
        ([(1408, 64, 8192)], 0, AMPLE, 0, {}, (0, 16, 8, 1, 1, 0, 0, 0, 88, 8, 1, 0)),              # 5: Versa's skinny long-K projection
        ([(11264, 64, 768)] * 3, TB | MASK, AMPLE, 0, {}, (0, 64, 1, 0, 1, 0, 0, 0, 176, 1, 3, 0)), # 6: dU
        ([(1408, 64, 768)] * 3, 0, AMPLE, 0, {}, (0, 16, 1, 0, 1, 0, 0, 0, 88, 1, 3, 0)),           # 7
        ([(1408, 1024, 64), (1408, 1024, 1024)], TB, AMPLE, 0, {}, (3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)),   # 8: a mixed group
        (cached6, DW, 0, 1, {}, (0, 64, 15, 0, 1, 1, 2, 0, 12, 15, 6, 0)),                          # 1 without scratch: tiled, atomics
        (cached6, DW, AMPLE, 1, {"gemm32_dw": 0}, (0, 64, 15, 2, 1, 1, 2, 0, 12, 15, 6, 0)),        # 1 with the weight-gradient kernel off
        (k64, 0, AMPLE, 0, {"gemm32_k64": 0}, (0, 64, 1, 0, 1, 0, 0, 0, 2112, 1, 3, 0)),            # 4 with the K = 64 kernel off
        # beyond the anchors
        (cached6, DW, 100000, 1, {}, (0, 64, 7, 0, 1, 1, 2, 0, 12, 7, 6, 0)),                       # scratch too small for the partials
        (cached6, DW, AMPLE, 1, {"gemm32_dw_splits": 5}, (2, 64, 5, 2, 0, 0, 1, 0, 12, 5, 6, 0)),
        ([(64, 768, 11264)] * 3, DW, AMPLE, 0, {}, (2, 64, 7, 2, 0, 0, 0, 0, 12, 7, 3, 0)),         # no column sums wanted
        ([(1024, 1024, 1408)], DW, AMPLE, 0, {}, (2, 64, 1, 2, 0, 0, 0, 0, 256, 1, 1, 0)),          # tiles fill the chip: ONE split, still gemm32_dw
        ([(64, 64, 1408), (64, 64, 11264)], DW, AMPLE, 1, {}, (2, 64, 11, 2, 0, 0, 1, 0, 1, 11, 2, 0)),     # splits follow the shortest K
        ([(100, 64, 1408)], DW, AMPLE, 0, {}, (0, 64, 11, 2, 0, 0, 0, 0, 2, 11, 1, 0)),             # M % 64: tiled, partials through the scratch
        ([(64, 768, 1408)], DW, 0, 0, {}, (0, 64, 11, 0, 1, 0, 0, 0, 12, 11, 1, 0)),                # iisan_linear_bwd: no executor, no scratch
        ([(64, 64, 1408)], TA | TB, 0, 1, {}, (0, 16, 1, 0, 1, 0, 2, 0, 4, 1, 1, 0)),
        ([(1408, 64, 8192)], 0, 0, 0, {}, (0, 16, 1, 0, 1, 0, 0, 0, 88, 1, 1, 0)),                  # 5 without scratch: never split
        (k64, TB, AMPLE, 0, {}, (1, 0, 0, 0, 0, 0, 0, 4, 176, 3, 3, 0)),
        ([(130, 768, 64)], TB, 0, 0, {}, (1, 0, 0, 0, 0, 0, 0, 1, 3, 12, 1, 0)),                    # a small launch: one column block per workgroup
        ([(1408, 256, 64)] * 5, 0, AMPLE, 0, {}, (0, 32, 1, 0, 1, 0, 0, 0, 176, 1, 5, 0)),          # the K = 64 kernel takes four problems
        ([(1408, 256, 768)] * 3, GELU | PREACT, AMPLE, 0, {}, (0, 32, 1, 0, 1, 0, 0, 0, 176, 1, 3, 0)),
        ([(70, 64, 48)], 0, 0, 0, {}, (0, 16, 1, 0, 0, 0, 0, 0, 5, 1, 1, 0)),                       # ragged: the generic fetch
        ([(64, 64, 64)] * 7, 0, 0, 0, {}, None),                                                    # more than six problems: rejected
    ]
    for probs, flags, scratch, colsum, knobs, want in table:
        n = len(probs)
        M = (C.c_int64 * n)(*[q[0] for q in probs])
        N = (C.c_int32 * n)(*[q[1] for q in probs])
        K = (C.c_int64 * n)(*[q[2] for q in probs])
        out = (C.c_int32 * 12)()
        with _lib.dev(**knobs):
            rc = lib.iisan_gemm32_plan(M, N, K, n, flags, scratch, colsum, out)
        if want is None:
            assert rc < 0, (probs, flags, rc)
        else:
            assert rc == want[0] and tuple(out) == want, (probs, flags, scratch, colsum, knobs, rc, tuple(out), want)


def test_encoder_plan_table():
    """What the two encoder executors decide once per call, before their first launch (encoders.hip: vit_plan / bert_plan, asked through
    `iisan_encoder_plan` without weights, workspace or device), as a literal table.  ViT: R = fp32 stream of the dev switch resid32, I = mixed
    stream + LayerNorm images, F = LayerNorm in the QKV / FC1 epilogues, S = ... and the residual adds in the O / FC2 epilogues; then f = the
    FC1 -> FC2 intermediate is block-major, x = the stream is, w = the call folds the LayerNorm weights itself.  BERT: M = mixed stream (P: fp32),
    a = stream and 16-bit image share a buffer, f as above.  ! = the executors refuse the sizes.  Columns: gemm16_variant 0, then 4, each under
    ln_fold 0 / 1 / 2 x blk32 0 / 1 / 2; then resid32 = 1 under gemm16_variant 0 and 4.  Expected values: recorded from the three probe functions
    this plan replaced (vit_strategy, f1_blk32, x16_blk32, called as the executors called them, in an instrumented build of the parent commit);
    they agree with every anchor derived by hand from that code, asserted again below.  The routes depend on `iisan_cu_count` through
    gemm16_route's half-a-tile-per-CU rule at 256 compute units: an MI355X, and what the library assumes where no device is visible."""
    from iisan_amd import _lib
    lib = _lib.load()
    VIT, BERT, F16, BF16 = 0, 1, 0, 1
    knobs = [dict(ln_fold=l, blk32=b, gemm16_variant=v) for v in (0, 4) for l in (0, 1, 2) for b in (0, 1, 2)] + \
            [dict(resid32=1, gemm16_variant=v) for v in (0, 4)]
    # (tower, dtype16, hidden, heads, mlp, tokens, M, chunk_items, deepest tap, full_blocks, folded set supplied) -> plan under each knob set
    table = [
        ((0, 0, 768, 12, 3072, 197, 1408, 0, 12, 0, 1), "I If If F Ff Ff S Sf Sfx I If If F Ff Ff S Sf Sfx R R"),
        ((0, 0, 768, 12, 3072, 197, 1408, 1000, 12, 0, 1), "I If If F Ff Ff S Sf Sfx I If If F Ff Ff S Sf Sfx R R"),
        ((1, 0, 768, 12, 3072, 30, 1408, 0, 12, 0, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((1, 0, 768, 12, 3072, 30, 1408, 1000, 12, 0, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((0, 1, 768, 12, 3072, 197, 1408, 0, 12, 0, 1), "I If If I If If I If If I If If I If If I If If R R"),
        ((0, 1, 768, 12, 3072, 197, 1408, 1000, 12, 0, 1), "I If If I If If I If If I If If I If If I If If R R"),
        ((1, 1, 768, 12, 3072, 30, 1408, 0, 12, 0, 0), "M Mf Mf M Mf Mf M Mf Mf M Mf Mf M Mf Mf M Mf Mf Pf Pf"),
        ((1, 1, 768, 12, 3072, 30, 1408, 1000, 12, 0, 0), "M Mf Mf M Mf Mf M Mf Mf M Mf Mf M Mf Mf M Mf Mf Pf Pf"),
        ((0, 0, 768, 12, 3072, 197, 1408, 0, 12, 0, 0), "I If If Fw Ffw Ffw Sw Sfw Sfxw I If If Fw Ffw Ffw Sw Sfw Sfxw R R"),
        ((0, 0, 768, 12, 3072, 197, 4, 0, 12, 0, 1), "I I I I I I I I I I If If F Ff Ff S Sf Sfx R R"),
        ((1, 0, 768, 12, 3072, 30, 4, 0, 12, 0, 0), "M M M Ma Ma Ma Ma Ma Ma M Mf Mf Ma Maf Maf Ma Maf Maf P Pf"),
        ((0, 0, 768, 12, 3072, 577, 1408, 0, 12, 0, 1), "I If If F Ff Ff S Sf Sfx I If If F Ff Ff S Sf Sfx R R"),
        ((1, 0, 768, 12, 3072, 577, 1408, 0, 12, 0, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((0, 0, 1024, 16, 4096, 197, 1408, 0, 24, 0, 1), "I If If I If If I If If I If If I If If I If If R R"),
        ((0, 0, 384, 6, 1536, 197, 1408, 0, 12, 0, 1), "I I I I I I I I I I I I I I I I I I R R"),
        ((0, 0, 192, 3, 768, 197, 1408, 0, 12, 0, 1), "I I I I I I I I I I I I I I I I I I R R"),
        ((1, 0, 1024, 16, 4096, 30, 1408, 0, 24, 0, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((1, 0, 256, 4, 1024, 30, 1408, 0, 4, 0, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((1, 0, 128, 2, 512, 30, 1408, 0, 2, 0, 0), "M M M Ma Ma Ma Ma Ma Ma M M M Ma Ma Ma Ma Ma Ma P P"),
        ((0, 0, 768, 12, 3072, 197, 1408, 0, 0, 0, 1), "I If If I If If I If If I If If I If If I If If R R"),
        ((1, 0, 768, 12, 3072, 30, 1408, 0, 0, 0, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((0, 0, 768, 12, 3072, 197, 1408, 0, 6, 0, 1), "I If If F Ff Ff S Sf Sfx I If If F Ff Ff S Sf Sfx R R"),
        ((0, 0, 768, 12, 3072, 197, 1408, 0, 6, 1, 1), "I If If F Ff Ff S Sf Sfx I If If F Ff Ff S Sf Sfx R R"),
        ((0, 0, 768, 12, 3072, 197, 1408, 1000, 6, 1, 1), "I If If F Ff Ff S Sf Sfx I If If F Ff Ff S Sf Sfx R R"),
        ((1, 0, 768, 12, 3072, 30, 1408, 0, 6, 1, 0), "M Mf Mf Ma Maf Maf Ma Maf Maf M Mf Mf Ma Maf Maf Ma Maf Maf Pf Pf"),
        ((0, 0, 768, 12, 3072, 1025, 1408, 0, 12, 0, 1), "! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! !"),
        ((1, 0, 768, 12, 3072, 0, 1408, 0, 12, 0, 0), "! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! !"),
        ((0, 0, 768, 12, 3072, 197, 0, 0, 12, 0, 1), "! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! !"),
        ((0, 0, 512, 8, 2048, 197, 1408, 0, 12, 0, 1), "! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! ! !"),
    ]

    def code(tower, w):
        if w < 0:
            return "!"
        if tower == VIT:
            return "RIFS"[w & 3] + ("f" if w & 4 else "") + ("x" if w & 8 else "") + ("w" if w & 16 else "")
        return ("M" if w & 1 else "P") + ("a" if w & 2 else "") + ("f" if w & 4 else "")

    def plan(case, **kn):
        with _lib.dev(**kn):
            return code(case[0], lib.iisan_encoder_plan(*case))

    for case, want in table:
        got = [plan(case, **kn) for kn in knobs]
        assert got == want.split(), (case, " ".join(got), want)
    # the anchors: ViT-B and BERT-base at the bs = 128 headline batch of 1,408 items
    vit = lambda dt=F16, hidden=768, heads=12, M=1408, tap=12: (VIT, dt, hidden, heads, 4 * hidden, 197, M, 0, tap, 0, 1)
    assert plan(vit()) == "Sfx"
    assert plan(vit(BF16)) == "If"                                   # LayerNorm in the epilogue is fp16 only
    assert plan(vit(), resid32=1) == "R"
    for hidden, heads in ((1024, 16), (384, 6), (192, 3)):
        assert plan(vit(hidden=hidden, heads=heads))[0] == "I"       # the folded routes are 768 wide
    assert plan(vit(), ln_fold=0) == "If" and plan(vit(), ln_fold=1) == "Ff"
    assert plan(vit(), blk32=0) == "S" and plan(vit(), blk32=1) == "Sf"
    assert plan(vit(tap=0))[0] == "I"                                # taps [0] only: no live block
    assert plan(vit(M=4)) == "I"                                     # below half a tile per CU the products run on the 128x128 kernel
    bert = lambda dt: (BERT, dt, 768, 12, 3072, 30, 1408, 0, 12, 0, 0)
    assert plan(bert(F16)) == "Maf" and plan(bert(BF16)) == "Mf"


def test_tools_compile_and_name_only_declared_entry_points():
    """a development tool that still iterated a table the ABI clean-up had removed died silently in every child process.  Every
    script under tools/ must byte-compile, and every `iisan_*` entry point it names must be one the loader binds (`_lib.SIGNATURES` =
    the symbols include/iisan_hip.h declares); attributes of `_lib` it touches must exist."""
    import glob
    import py_compile
    import re
    from iisan_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for path in sorted(glob.glob(os.path.join(root, "tools", "*.py"))):
        py_compile.compile(path, doraise=True)
        src = open(path).read()
        for name in set(re.findall(r"\biisan_[a-z0-9_]+\b", src)):
            if name in ("iisan_amd", "iisan_hip", "iisan_oracle"):
                continue
            assert name in _lib.SIGNATURES, f"{os.path.basename(path)} names {name}, which the library does not export"
        for attr in set(re.findall(r"\b_lib\.([A-Za-z_]+)\b", src)):
            assert hasattr(_lib, attr), f"{os.path.basename(path)} uses _lib.{attr}, which does not exist"
