"""CPU restatement of timm's patch-8 ViT forward (``timm.create_model("vit_small_patch8_224" | "vit_base_patch8_224", num_classes=0)``)
in plain torch functional ops, over the state dict of effocr_amd.weights (timm key names).  Written from the architecture (Dosovitskiy et
al. 2020 as timm builds it): an 8x8 / stride-8 patch convolution, a class token, a learned position embedding, pre-norm blocks (LayerNorm
eps 1e-6, a qkv linear WITH bias, softmax(q k^T / 8) v at head dim 64, exact erf GELU, MLP ratio 4), a final LayerNorm, the class-token
row as the pooled output.  It takes its geometry from the tensors it is given, not from ``param_shapes``.  The GPU tests compare the HIP
encoder against it; tests/test_vit8_host.py pins it to an independent implementation, transformers' ViTModel(patch_size=8).  It reads
nothing outside the repository.

``attention_ref`` and ``attention_emulated`` are the references of the attention operator's tests: the exact value in float64, and the
same value with the rounding points that csrc/vit8.hpp declares for the 16-bit kernel, computed without a GPU."""
import torch
import torch.nn.functional as F

from effocr_amd.weights import strip_prefix

EPS = 1e-6
HEAD_DIM = 64
PATCH = 8
KEY_TILE_16BIT = 64          # VIT8_KTILE16 of csrc/vit8.hpp: the 16-bit kernel rescales once per 64 keys


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def attention_ref(q, k, v):
    """q, k, v [..., T, 64] -> softmax(q k^T / 8) v in float64."""
    q, k, v = q.double(), k.double(), v.double()
    return (q @ k.transpose(-2, -1) / HEAD_DIM ** 0.5).softmax(-1) @ v


def attention_emulated(q, k, v, dtype, key_tile=KEY_TILE_16BIT):
    """The same value with the 16-bit kernel's declared rounding points and nothing else: q, k, v as given (already in ``dtype``); the
    key tiles walked in ascending order with a running maximum m and sum l; per tile p = exp((s - m') / 8) ROUNDED to ``dtype`` for the
    P V product while l sums the unrounded p; O / l rounded once to ``dtype``.  Everything between the rounding points is float64, so the
    distance of this from attention_ref is the error the number format alone forces on the kernel."""
    q, k, v = q.double(), k.double(), v.double()
    T = q.shape[-2]
    m = torch.full(q.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for k0 in range(0, T, key_tile):
        s = q @ k[..., k0:k0 + key_tile, :].transpose(-2, -1) / HEAD_DIM ** 0.5
        mn = torch.maximum(m, s.amax(-1, keepdim=True))
        alpha = torch.exp(m - mn)
        p = torch.exp(s - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(dtype).double() @ v[..., k0:k0 + key_tile, :]
        m = mn
    return (o / l).to(dtype).double()


def split_qkv(qkv, B, T, heads):
    """qkv [B*T, 3*heads*64] (q | k | v, feature = which * D + h * 64 + d) -> q, k, v [B, heads, T, 64]."""
    return qkv.view(B, T, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)


def merge_heads(o):
    """[B, heads, T, 64] -> [B*T, heads*64] (feature = h * 64 + d)."""
    B, heads, T, _ = o.shape
    return o.transpose(1, 2).reshape(B * T, heads * HEAD_DIM)


def patch_embed(x, w, b, cls, pos):
    """x [B,3,S,S], w [D,3,8,8], b [D], cls [1,1,D], pos [1,T,D] -> tokens [B, T, D]: cls + pos[0], then conv(x)[p] + b + pos[1 + p]."""
    h = F.conv2d(x, w, b, stride=PATCH).flatten(2).transpose(1, 2)
    return torch.cat([cls.expand(x.shape[0], -1, -1), h], dim=1) + pos


def vit8_forward(sd, x):
    """x [B,3,S,S] (S a multiple of 8, float64 or float32) -> norm(tokens)[:, 0], [B, D] in x's dtype.  Width, depth and heads are read
    from the tensors: D from cls_token, depth from the block keys, heads = D / 64."""
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}
    D = P["cls_token"].shape[-1]
    heads = D // HEAD_DIM
    depth = 1 + max(int(k.split(".")[1]) for k in P if k.startswith("blocks."))
    h = patch_embed(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], P["cls_token"], P["pos_embed"])
    B, T, _ = h.shape
    for i in range(depth):
        p = f"blocks.{i}."
        y = _ln(h, P[p + "norm1.weight"], P[p + "norm1.bias"])
        qkv = F.linear(y, P[p + "attn.qkv.weight"], P[p + "attn.qkv.bias"])
        q, k, v = split_qkv(qkv.reshape(B * T, 3 * D), B, T, heads)
        o = (q @ k.transpose(-2, -1) / HEAD_DIM ** 0.5).softmax(-1) @ v
        h = h + F.linear(o.transpose(1, 2).reshape(B, T, D), P[p + "attn.proj.weight"], P[p + "attn.proj.bias"])
        y = _ln(h, P[p + "norm2.weight"], P[p + "norm2.bias"])
        h = h + F.linear(F.gelu(F.linear(y, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"])
    return _ln(h[:, 0], P["norm.weight"], P["norm.bias"])


def logits(sd, x):
    """vit8_forward + timm's classifier head."""
    P = strip_prefix(sd)
    return F.linear(vit8_forward(sd, x), P["head.weight"].to(x.dtype), P["head.bias"].to(x.dtype))


def hf_config(D, depth, heads, img_size):
    """The transformers ViTConfig of a patch-8 ViT: eps 1e-6, exact GELU, qkv bias, eager attention."""
    from transformers import ViTConfig
    return ViTConfig(hidden_size=D, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=4 * D, image_size=img_size,
                     patch_size=PATCH, layer_norm_eps=EPS, hidden_act="gelu", qkv_bias=True, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, attn_implementation="eager")


def hf_state_dict(sd, hf_keys):
    """timm key names -> the key names of the installed transformers ViTModel (``hf_keys``: its state-dict keys).  Two layouts exist:
    ``layers.i.attention.{q,k,v,o}_proj`` / ``mlp.fc1`` and the older ``encoder.layer.i.attention.attention.{query,key,value}`` /
    ``attention.output.dense`` / ``intermediate.dense`` / ``output.dense``; q, k and v are split out of qkv in both."""
    new = any(k.startswith("layers.") for k in hf_keys)
    out = {}
    for k, v in strip_prefix(sd).items():
        leaf = k.rsplit(".", 1)[-1]
        if k.startswith("head."):
            continue
        if k == "cls_token":
            out["embeddings.cls_token"] = v
        elif k == "pos_embed":
            out["embeddings.position_embeddings"] = v
        elif k.startswith("patch_embed.proj."):
            out["embeddings.patch_embeddings.projection." + leaf] = v
        elif k.startswith("norm."):
            out["layernorm." + leaf] = v
        else:
            parts = k.split(".")
            i, rest = parts[1], ".".join(parts[2:-1])
            pre = f"layers.{i}." if new else f"encoder.layer.{i}."
            if rest == "attn.qkv":
                names = ("q_proj", "k_proj", "v_proj") if new else ("attention.query", "attention.key", "attention.value")
                for n, t in zip(names, v.chunk(3, dim=0)):
                    out[pre + f"attention.{n}.{leaf}"] = t.clone()
            else:
                m = ({"attn.proj": "attention.o_proj", "norm1": "layernorm_before", "norm2": "layernorm_after", "mlp.fc1": "mlp.fc1",
                      "mlp.fc2": "mlp.fc2"} if new else
                     {"attn.proj": "attention.output.dense", "norm1": "layernorm_before", "norm2": "layernorm_after",
                      "mlp.fc1": "intermediate.dense", "mlp.fc2": "output.dense"})
                out[pre + m[rest] + "." + leaf] = v
    return out
