"""The arithmetic of a CLIP vision tower restated in float64, and the seeded inputs of the HuggingFace golden `tests/golden/clip_vit.npz`
(tests/golden/make_clip_golden.py) that both sides rebuild.

A CLIP vision transformer (HF `CLIPVisionTransformer`) is the pre-LN ViT of `oracle/iisan_oracle.py` with four differences: a LayerNorm
between the embeddings and block 0 (`pre_layrnorm`; `hidden_states[0]` is its OUTPUT), quick-GELU `x * sigmoid(1.702 x)` in the MLP when
`config.hidden_act` says so, no bias on the patch convolution, eps 1e-5.  `post_layernorm` touches the pooled output only."""
import hashlib
import os

import numpy as np
import torch
import torch.nn.functional as F

from iisan_amd import weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_vit.npz")

# the towers of the golden: CLIP-B/32 at full size (50 tokens); an L/14-shaped toy (hidden 1024 = 16 x 64, 14-pixel patches: the padded patch
# extraction, 2 x 2 patches + CLS = 5 tokens); a toy whose config says "gelu" (the LAION checkpoints: the erf form behind the pre-LayerNorm)
_CLIP = dict(eps=1e-5, pre_ln=True, patch_bias=False)
TOWERS = {
    "b32": (weights.CLIP_VIT_B32, 51, 52, 4),
    "l14toy": (weights.VitConfig(hidden=1024, layers=2, heads=16, mlp=4096, image=28, patch=14, act="quick_gelu", **_CLIP), 53, 54, 4),
    "gelutoy": (weights.VitConfig(hidden=768, layers=2, heads=12, mlp=512, image=32, patch=16, act="gelu", **_CLIP), 55, 56, 4),
}       # name: (config, weight seed, image seed, items)


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def images(n: int, res: int, seed: int) -> torch.Tensor:
    """n seeded images in [-1, 1] (the normalised range), the first one all zero: the padding item the reference ships."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, res, res, generator=g).clamp_(-1.0, 1.0)
    x[0] = 0
    return x


def tower_inputs(name: str):
    """(config, canonical weights, images) of one tower of the golden."""
    cfg, seed_w, seed_x, n = TOWERS[name]
    return cfg, weights.make_vit_weights(cfg, seed=seed_w), images(n, cfg.image, seed_x)


def load_golden(name: str):
    """(config, weights, images, expected CLS rows [items, layers + 1, D] of HF's hidden states) — the seeded inputs checked against the
    checksums the generator stored."""
    z = np.load(GOLDEN)
    cfg, w, x = tower_inputs(name)
    assert str(z[name + "_images_sha"]) == sha(x) and str(z[name + "_w_sha"]) == sha(w["L1.fc2_w"]), "the seeded inputs are not those of the golden"
    return cfg, w, x, torch.from_numpy(z[name + "_taps"])


def quick_gelu(x: torch.Tensor) -> torch.Tensor:
    return x * torch.sigmoid(1.702 * x)


def _patches(images: torch.Tensor, p: int) -> torch.Tensor:
    B, C, H, W = images.shape
    return images.view(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B, (H // p) * (W // p), C * p * p)


def _mha(x, qkv_w, qkv_b, heads):
    B, S, D = x.shape
    d = D // heads
    qkv = F.linear(x, qkv_w, qkv_b).view(B, S, 3, heads, d)
    q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * (d ** -0.5), dim=-1)
    return torch.matmul(p, v).transpose(1, 2).reshape(B, S, D)


def clip_hidden_states(images: torch.Tensor, w, cfg, dtype=torch.float64, round16=None):
    """All layers + 1 hidden states [B, T, D] of the tower in `dtype`.  round16 (a torch dtype): every GEMM operand — activations and
    weights — is rounded to it first, everything else stays in `dtype`: the emulation of the kernels' 16-bit operand rounding alone
    (DESIGN 3), the yardstick the measured tap errors are read against."""
    r = (lambda t: t.to(round16).to(dtype)) if round16 is not None else (lambda t: t)
    w = {k: v.to(dtype) for k, v in w.items()}
    lin = lambda t, W, b: F.linear(r(t), r(W), b)
    B, D = images.shape[0], cfg.hidden
    act = quick_gelu if cfg.act == "quick_gelu" else F.gelu
    x = lin(_patches(images.to(dtype), cfg.patch), w["patch_w"], w.get("patch_b"))
    x = torch.cat([w["cls_token"].view(1, 1, -1).expand(B, -1, -1), x], dim=1) + w["pos_emb"][None]
    if cfg.pre_ln:
        x = F.layer_norm(x, (D,), w["pre_ln_w"], w["pre_ln_b"], cfg.eps)
    hs = [x]
    for l in range(cfg.layers):
        p = f"L{l}."
        h = F.layer_norm(x, (D,), w[p + "ln1_w"], w[p + "ln1_b"], cfg.eps)
        if round16 is None:
            a = _mha(h, w[p + "qkv_w"], w[p + "qkv_b"], cfg.heads)
        else:       # q, k, v and the probabilities are 16-bit operands of the attention products too
            B_, S, _ = h.shape
            d = D // cfg.heads
            qkv = r(lin(h, w[p + "qkv_w"], w[p + "qkv_b"])).view(B_, S, 3, cfg.heads, d)
            q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
            pr = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * (d ** -0.5), dim=-1)
            a = torch.matmul(r(pr), v).transpose(1, 2).reshape(B_, S, D)
        x = x + lin(a, w[p + "o_w"], w[p + "o_b"])
        h = F.layer_norm(x, (D,), w[p + "ln2_w"], w[p + "ln2_b"], cfg.eps)
        x = x + lin(act(lin(h, w[p + "fc1_w"], w[p + "fc1_b"])), w[p + "fc2_w"], w[p + "fc2_b"])
        hs.append(x)
    return hs


def clip_cls_taps(images: torch.Tensor, w, cfg, dtype=torch.float64, round16=None) -> torch.Tensor:
    """[B, layers + 1, D]: the CLS row of every hidden state."""
    return torch.stack([h[:, 0] for h in clip_hidden_states(images, w, cfg, dtype, round16)], dim=1)


def tap_errors(got: torch.Tensor, ref: torch.Tensor):
    """per tap layer: |got - ref| / |ref| in the 2-norm over the items — the measure of test_full_size_taps_match_reference_golden"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return [float((got[:, l] - ref[:, l]).norm() / ref[:, l].norm()) for l in range(ref.shape[1])]
