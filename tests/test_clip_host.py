"""CLIP vision towers, the part that needs no GPU: the float64 restatement against HuggingFace's own outputs, the state-dict key map, the
C struct, the executor's plan for a CLIP tower, the routing of the quick-GELU epilogue (mode 8) and the register budget of its 256x256
instantiations.  The GPU side is tests/test_gpu_clip.py."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import clip_oracle as CO
from iisan_amd import _lib, weights

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "iisan_amd", "csrc")
F16, BF16 = _lib.IISAN_F16, _lib.IISAN_BF16
GELU16, QGELU16 = _lib.EPI_GELU16, _lib.EPI_QGELU16
V1, H256, REJECTED = 0, 2, -1


@pytest.mark.parametrize("name", sorted(CO.TOWERS))
def test_float64_restatement_matches_the_huggingface_golden(name):
    """`clip_oracle.clip_cls_taps` against `hidden_states[l][:, 0]` of HF's CLIPVisionModel (fp32), every layer, at the 2e-5 the
    oracle-vs-golden tests use: the pre-LayerNorm IS hidden state 0, quick-GELU or erf-GELU by the config, no patch bias."""
    cfg, w, x, gold = CO.load_golden(name)
    assert "patch_b" not in w and "pre_ln_w" in w and gold.shape == (x.shape[0], cfg.layers + 1, cfg.hidden)
    got = CO.clip_cls_taps(x, w, cfg)
    err, ref = (got - gold.double()).abs().max().item(), gold.abs().max().item()
    assert err <= 2e-5 + 2e-5 * ref, f"{name}: max|err| {err:.3e} vs scale {ref:.3e}"
    # ... and the restatement is not the plain ViT's: without the pre-LayerNorm, or with the other activation, it is far off the golden
    other = weights.VitConfig(**{**weights.config_dict(cfg), "act": "gelu" if cfg.act == "quick_gelu" else "quick_gelu"})
    assert (CO.clip_cls_taps(x, w, other)[:, 1:] - gold[:, 1:].double()).abs().max().item() > 1e-3
    no_pre = weights.VitConfig(**{**weights.config_dict(cfg), "pre_ln": False})
    assert (CO.clip_cls_taps(x, w, no_pre)[:, 0] - gold[:, 0].double()).abs().max().item() > 1e-2


def test_clip_vit_from_hf_round_trips_both_key_prefixes():
    cfg = weights.VitConfig(hidden=128, layers=2, heads=2, mlp=256, image=32, patch=16, eps=1e-5, pre_ln=True, act="quick_gelu", patch_bias=False)
    w = weights.make_vit_weights(cfg, seed=3)
    assert "patch_b" not in w and {"pre_ln_w", "pre_ln_b"} <= set(w)
    # the tensors a CLIP config shares with a plain ViT config of the same shape are the same draws
    plain = weights.make_vit_weights(weights.VitConfig(hidden=128, layers=2, heads=2, mlp=256, image=32, patch=16), seed=3)
    assert all(torch.equal(w[k], plain[k]) for k in w if k in plain) and "patch_b" in plain and "pre_ln_w" not in plain
    for prefix in ("vision_model.", ""):
        sd = weights.clip_vit_to_hf(w, cfg, prefix)
        assert all(k.startswith(prefix) for k in sd) and prefix + "pre_layrnorm.weight" in sd
        assert sd[prefix + "embeddings.patch_embedding.weight"].shape == (128, 3, 16, 16) and prefix + "embeddings.patch_embedding.bias" not in sd
        # what a checkpoint carries beside the tower is dropped: post_layernorm, position ids, a projection, the text tower of a CLIPModel
        sd[prefix + "post_layernorm.weight"] = torch.ones(128)
        sd[prefix + "post_layernorm.bias"] = torch.zeros(128)
        sd[prefix + "embeddings.position_ids"] = torch.arange(5)[None]
        sd["visual_projection.weight"] = torch.zeros(64, 128)
        if prefix:
            sd["text_model.embeddings.position_embedding.weight"] = torch.zeros(7, 128)
        back = weights.clip_vit_from_hf(sd)
        assert set(back) == set(w) - {"lnf_w", "lnf_b"}
        assert all(torch.equal(back[k], w[k]) for k in back)
    # the named constants
    assert (weights.CLIP_VIT_B32.tokens, weights.CLIP_VIT_B16.tokens, weights.CLIP_VIT_L14.tokens) == (50, 197, 257)
    assert weights.CLIP_VIT_L14.hidden == 1024 and weights.CLIP_VIT_L14.patch_ld == 640 and weights.CLIP_VIT_B32.eps == 1e-5
    assert weights.CLIP_VIT_B32.norm_mean is None and weights.VIT_BASE.pre_ln is False and weights.VIT_BASE.act == "gelu"
    with pytest.raises(ValueError):
        weights.VitConfig(act="relu")


def test_vit_weights_struct_carries_the_clip_fields_where_c_puts_them(tmp_path):
    """The ctypes mirror against gcc's layout of the new trailing fields (tests/test_abi.py compares the sizes)."""
    src = tmp_path / "l.c"
    fields = ("folded", "pre_ln_w", "pre_ln_b", "act", "norm_mean", "norm_std")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "iisan_hip.h"\nint main(){printf("%zu' + " %zu" * len(fields) + '\\n",sizeof(iisan_vit_weights),'
                   + ",".join(f"offsetof(iisan_vit_weights,{f})" for f in fields) + ');return 0;}\n')
    exe = tmp_path / "l"
    subprocess.check_call(["gcc", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.VitWeights)] + [getattr(_lib.VitWeights, f).offset for f in fields]
    z = _lib.VitWeights()
    assert not z.pre_ln_w and z.act == 0 and list(z.norm_mean) == [0.0] * 3 and list(z.norm_std) == [0.0] * 3       # zero = today's ViT


def test_encoder_plan_answers_for_a_clip_tower(lib):
    """IISAN_TOWER_CLIP = 2: the ViT executor's decision for a CLIP tower, the ViT bit meanings.  Never the folded routes (bits 0-1 stay 1:
    mixed stream + LayerNorm images; never 8 or 16), at 768 with fp16 operands included — where the plain ViT of the same sizes takes them;
    the block-major FC1 -> FC2 intermediate (4) wherever FC1 and FC2 reach the 256x256 kernel, quick-GELU epilogue and all."""
    plan = lambda tower, dt, D, H, F, T, M, folded=0: lib.iisan_encoder_plan(tower, dt, D, H, F, T, M, 0, 12, 0, folded)
    VIT, CLIP = _lib.IISAN_TOWER_VIT, _lib.IISAN_TOWER_CLIP
    assert plan(VIT, F16, 768, 12, 3072, 50, 1408, 1) == (3 | 4 | 8)            # the product route of the plain ViT
    assert plan(CLIP, F16, 768, 12, 3072, 50, 1408, 1) == (1 | 4)
    assert plan(CLIP, F16, 768, 12, 3072, 50, 1408, 0) == (1 | 4)               # ... and no call-time fold either
    assert plan(CLIP, BF16, 768, 12, 3072, 197, 1408) == (1 | 4)
    assert plan(CLIP, F16, 1024, 16, 4096, 257, 1408) == (1 | 4)                # ViT-L/14
    assert plan(CLIP, F16, 768, 12, 3072, 50, 4) == 1                           # a small batch: the 128x128 kernel, row-major F1
    assert plan(CLIP, F16, 1280, 16, 5120, 257, 64) & 32                        # 80-wide heads as for a ViT
    with _lib.dev(resid32=1):
        assert plan(CLIP, F16, 768, 12, 3072, 50, 1408) & 3 == 0
    for lf in (0, 1, 2):
        with _lib.dev(ln_fold=lf):
            assert plan(CLIP, F16, 768, 12, 3072, 50, 1408, 1) == (1 | 4)
    # the refusals are the ViT's
    assert plan(CLIP, F16, 512, 8, 2048, 50, 8) < 0 and plan(CLIP, F16, 1280, 20, 5120, 257, 8) < 0 and plan(CLIP, F16, 768, 12, 3072, 1025, 8) < 0
    assert lib.iisan_encoder_plan(3, F16, 768, 12, 3072, 50, 8, 0, 12, 0, 0) < 0


def test_mode_8_is_routed_wherever_mode_1_is(lib):
    route = lambda dt, mode, M, N, K, ob=0, rowstat=0, ab=0: lib.iisan_gemm16_route_blk32(dt, mode, M, N, K, 0, 0, 0, rowstat, ab, ob)
    shapes = [(1, 128, 64), (37, 192, 128), (300, 192, 64), (300, 576, 192), (9800, 3072, 768), (70400, 3072, 768), (277376, 3072, 768), (1300, 4096, 1024)]
    for variant in (0, 1, 4):
        with _lib.dev(gemm16_variant=variant):
            for dt in (F16, BF16):
                for M, N, K in shapes:
                    assert route(dt, QGELU16, M, N, K) == route(dt, GELU16, M, N, K) >= 0, (variant, dt, M, N, K)
                    assert route(dt, QGELU16, M, N, K, ob=1) == route(dt, GELU16, M, N, K, ob=1), (variant, dt, M, N, K)
    # the smallest products the auto policy sends to the 256x256 kernel: half a tile per CU = 128 tiles (256 compute units)
    assert route(F16, QGELU16, 127 * 256 + 1, 256, 128) == H256 and route(F16, QGELU16, 127 * 256, 256, 128) == V1
    assert route(F16, QGELU16, 127 * 256 + 1, 256, 128, ob=1) == H256 and route(F16, QGELU16, 127 * 256, 256, 128, ob=1) == REJECTED
    # the dev-only race screen has no mode 8: under variant 3 the 128x128 kernel takes what the staggered kernel takes in mode 1
    with _lib.dev(gemm16_variant=3):
        assert route(F16, GELU16, 70400, 3072, 768) == 1 and route(F16, QGELU16, 70400, 3072, 768) == V1
    # no LayerNorm in the epilogue and no block-major A operand with it; mode 9 does not exist; ragged N from 768 on is refused as for mode 1
    assert route(F16, QGELU16, 70400, 3072, 768, rowstat=1) == REJECTED and route(F16, QGELU16, 70400, 3072, 768, ab=1) == REJECTED
    assert route(F16, 9, 300, 256, 128) == REJECTED and route(F16, QGELU16, 300, 832, 128) == REJECTED
    assert lib.iisan_gemm16_h256_applicable(QGELU16, 300, 512, 128, 0, 0, 0) == 1 and lib.iisan_gemm16_h256_applicable(QGELU16, 300, 384, 128, 0, 0, 0) == 0


def test_quick_gelu_instantiations_of_the_256_kernel_stay_inside_the_register_budget(tmp_path):
    """The four EPI_QGELU16 instantiations (both operand types, row-major and block-major output) live in gemm16_h256_qgelu.hip.  Each is held
    to the erf-GELU instantiation it stands beside — 248 VGPRs, no spilled SGPR at the parent commit (tests/test_blk32_host.py: PARENT) —
    with no scratch and no spilled VGPR: the activation is two transcendentals and one temporary per pair, fewer live registers than the fit."""
    import test_isa_screen as isa
    meta, txt = isa._kernel_meta(os.path.join(CSRC, "gemm16_h256_qgelu.hip"), tmp_path)
    seen = set()
    for name, m in meta.items():
        k = re.search(r"gemm16_h256_kernelI(3F16|4BF16)Li(\d)ELb([01])ELi(\d)EE", name)
        if not k:
            continue
        assert (int(k.group(2)), k.group(3)) == (QGELU16, "0"), name           # nothing but the mode's own instantiations
        seen.add((k.group(1), int(k.group(4))))
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0 and m["vgpr"] <= 248 and m["sgpr_spill"] == 0, (name, m)
    assert seen == {("3F16", 0), ("3F16", 2), ("4BF16", 0), ("4BF16", 2)}
    assert txt.count("v_exp_f32") > 0 and txt.count("v_rcp_f32") > 0
    assert not isa._opsel_sites(txt)


def test_clipvit_encoder_surface_and_mm_encoder_choice():
    """`MM_Encoder` builds a `ClipVit_Encoder` when 'clip-vit' is in args.CV_model_load (`Code_Uncached/model/encoders.py:9-12`); the class takes
    the tower as a FrozenVit on a CLIP config or as an HF-shaped module (a config + the HF state-dict keys, either prefix), owns the head as
    `classifier` where the reference's forward reads it, and exposes the same module as `image_net.classifier`."""
    from iisan_amd import factory
    from iisan_amd.model import encoders as menc
    cfg = weights.VitConfig(hidden=128, layers=2, heads=2, mlp=256, image=32, patch=16, eps=1e-5, pre_ln=True, act="quick_gelu", patch_bias=False)
    w = weights.make_vit_weights(cfg, seed=3)
    bcfg = weights.BertConfig(hidden=128, layers=2, heads=2, mlp=256, vocab=64, max_pos=16)
    bert = menc.FrozenBert(weights.make_bert_weights(bcfg, seed=4), bcfg)
    args = factory.make_args(CV_model_load="clip-vit-base-patch32", num_words_title=8)
    mm = menc.MM_Encoder(args, menc.FrozenVit(w, cfg, args.embedding_dim), bert)
    assert type(mm.cv_encoder) is menc.ClipVit_Encoder and mm.cv_encoder.n_layers == 2
    assert mm.cv_encoder.classifier is mm.cv_encoder.image_net.classifier
    assert "cv_encoder.image_net.classifier.weight" in dict(mm.named_parameters())
    args_vit = factory.make_args(num_words_title=8)
    plain = weights.VitConfig(hidden=128, layers=2, heads=2, mlp=256, image=32, patch=16)
    assert type(menc.MM_Encoder(args_vit, menc.FrozenVit(weights.make_vit_weights(plain, seed=3), plain, 64), bert).cv_encoder) is menc.Vit_Encoder
    with pytest.raises(ValueError):         # a plain ViT container is not a CLIP tower
        menc.ClipVit_Encoder(menc.FrozenVit(weights.make_vit_weights(plain, seed=3), plain, 64), 64)

    class HFShaped(torch.nn.Module):        # what the class reads of an HF CLIPVisionModel / CLIPVisionTransformer: .config and the state dict
        def __init__(self, prefix):
            super().__init__()
            self.config = type("Cfg", (), dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, image_size=32,
                                               patch_size=16, num_channels=3, layer_norm_eps=1e-5, hidden_act="quick_gelu"))()
            self._sd = weights.clip_vit_to_hf(w, cfg, prefix)

        def state_dict(self, *a, **k):
            return dict(self._sd, **{"classifier." + n: v for n, v in self.classifier.state_dict().items()}) if hasattr(self, "classifier") else dict(self._sd)

    for prefix in ("vision_model.", ""):
        e = menc.ClipVit_Encoder(image_net=HFShaped(prefix), item_dim=32)
        assert e.classifier is e.image_net.classifier and e.classifier.weight.shape == (32, 128)
        cw, ccfg = e._canonical()
        assert ccfg == cfg and set(cw) == set(w) - {"lnf_w", "lnf_b"} and all(torch.equal(cw[k], w[k]) for k in cw)
