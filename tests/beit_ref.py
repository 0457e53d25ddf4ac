"""CPU restatement of timm's BEiT forward (``timm.create_model("beit_base_patch16_224" | "beitv2_base_patch16_224", num_classes=0)``) in
plain torch functional ops, over the state dict of effocr_amd.weights (timm key names), written from the paper (Bao et al. 2021) and
timm's semantics: no absolute position embedding, a relative-position bias table per block with three extra rows for the cls token,
a qkv linear whose bias is [q_bias | 0 | v_bias], layer scale gamma_1 / gamma_2, LayerNorm eps 1e-6, exact GELU, and the pooled output
fc_norm(mean of the patch tokens).  The GPU tests compare the HIP encoder against it; tests/test_beit_host.py pins it to an independent
implementation, transformers' BeitModel.  It reads nothing outside the repository.

The keyword switches of ``beit_forward`` each plant ONE mistake a port could make; test_beit_host.py checks that the parity test sees
every one of them."""
import torch
import torch.nn.functional as F

from effocr_amd.weights import BEIT_CFG, PATCH, beit_relative_position_index, strip_prefix

EPS = 1e-6
HEAD_DIM = 64


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def bias_attention(q, k, v, table, W, swap_ij=False, swap_cls=False):
    """q, k, v [B, heads, T, 64] -> softmax(q k^T / 8 + table[index]) v, [B, heads, T, 64]; table [(2W-1)^2 + 3, heads]."""
    idx = beit_relative_position_index(W)
    if swap_ij:
        idx = idx.T
    if swap_cls:
        n = (2 * W - 1) ** 2
        idx = torch.where(idx == n, torch.full_like(idx, -1), idx)
        idx = torch.where(idx == n + 1, torch.full_like(idx, n), idx)
        idx = torch.where(idx == -1, torch.full_like(idx, n + 1), idx)
    T = idx.shape[0]
    bias = table[idx.flatten()].view(T, T, -1).permute(2, 0, 1)
    s = q @ k.transpose(-2, -1) / HEAD_DIM ** 0.5 + bias[None]
    return s.softmax(-1) @ v


def beit_forward(arch, sd, x, swap_ij=False, swap_cls=False, q_bias_on_k=False, k_bias_added=False, mean_with_cls=False, no_fc_norm=False):
    """x [B,3,S,S] (S a multiple of 16) -> pooled features [B, D] (dtype of x).  The planted mistakes: swap_ij (index[j, i]), swap_cls
    (rows (2W-1)^2 and (2W-1)^2 + 1 exchanged), q_bias_on_k (the bias vector packed [0 | q_bias | v_bias]: k is given q's bias),
    k_bias_added ([q_bias | q_bias | v_bias]: a bias on k on top of the right one on q — a constant per query, which softmax cancels),
    mean_with_cls, no_fc_norm."""
    D, depth, heads, _ = BEIT_CFG[arch]
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}
    B, W = x.shape[0], x.shape[-1] // PATCH
    T = W * W + 1
    h = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
    h = torch.cat([P["cls_token"].expand(B, -1, -1), h], dim=1)
    for i in range(depth):
        p = f"blocks.{i}."
        y = _ln(h, P[p + "norm1.weight"], P[p + "norm1.bias"])
        qb, zero = P[p + "attn.q_bias"], torch.zeros_like(P[p + "attn.q_bias"])
        bias = [zero, qb] if q_bias_on_k else [qb, qb] if k_bias_added else [qb, zero]
        qkv = F.linear(y, P[p + "attn.qkv.weight"], torch.cat(bias + [P[p + "attn.v_bias"]]))
        q, k, v = qkv.view(B, T, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4)
        o = bias_attention(q, k, v, P[p + "attn.relative_position_bias_table"], W, swap_ij, swap_cls)
        o = F.linear(o.transpose(1, 2).reshape(B, T, D), P[p + "attn.proj.weight"], P[p + "attn.proj.bias"])
        h = h + P[p + "gamma_1"] * o
        y = _ln(h, P[p + "norm2.weight"], P[p + "norm2.bias"])
        y = F.linear(F.gelu(F.linear(y, P[p + "mlp.fc1.weight"], P[p + "mlp.fc1.bias"])), P[p + "mlp.fc2.weight"], P[p + "mlp.fc2.bias"])
        h = h + P[p + "gamma_2"] * y
    pooled = (h if mean_with_cls else h[:, 1:]).mean(dim=1)
    return pooled if no_fc_norm else _ln(pooled, P["fc_norm.weight"], P["fc_norm.bias"])


def logits(arch, sd, x):
    """beit_forward + timm's classifier head."""
    P = strip_prefix(sd)
    return F.linear(beit_forward(arch, sd, x), P["head.weight"].to(x.dtype), P["head.bias"].to(x.dtype))


def hf_config(arch, img_size):
    """The transformers BeitConfig of ``arch`` at ``img_size``: relative-position bias per layer, mean pooling, no mask token, eps 1e-6."""
    from transformers import BeitConfig
    D, depth, heads, r = BEIT_CFG[arch]
    return BeitConfig(hidden_size=D, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=r * D, image_size=img_size,
                      patch_size=PATCH, use_mask_token=False, use_absolute_position_embeddings=False, use_relative_position_bias=True,
                      use_shared_relative_position_bias=False, use_mean_pooling=True, layer_norm_eps=EPS, hidden_act="gelu",
                      attn_implementation="eager")


def hf_state_dict(sd):
    """timm key names -> transformers BeitModel key names (q / k / v split out of qkv, q_bias / v_bias onto their projections, gamma ->
    lambda, fc_norm -> pooler.layernorm)."""
    out = {}
    for k, v in strip_prefix(sd).items():
        if k.startswith("head."):
            continue
        if k == "cls_token":
            out["embeddings.cls_token"] = v
        elif k.startswith("patch_embed.proj."):
            out["embeddings.patch_embeddings.projection." + k.rsplit(".", 1)[-1]] = v
        elif k.startswith("fc_norm."):
            out["pooler.layernorm." + k.rsplit(".", 1)[-1]] = v
        else:
            parts = k.split(".")
            pre, rest = f"layers.{parts[1]}.", ".".join(parts[2:])
            if rest == "attn.qkv.weight":
                for n, t in zip(("q_proj", "k_proj", "v_proj"), v.chunk(3, dim=0)):
                    out[pre + f"attention.{n}.weight"] = t.clone()
            elif rest in ("attn.q_bias", "attn.v_bias"):
                out[pre + f"attention.{rest[5]}_proj.bias"] = v
            else:
                out[pre + (rest.replace("gamma_", "lambda_").replace("attn.proj.", "attention.o_proj.")
                               .replace("attn.relative_position_bias_table", "relative_position_bias.relative_position_bias_table")
                               .replace("norm1.", "layernorm_before.").replace("norm2.", "layernorm_after."))] = v
    return out
