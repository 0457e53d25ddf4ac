"""CPU restatement of timm's Swin-T forward (``timm.create_model("swin_tiny_patch4_window7_224", num_classes=0)``) in plain torch functional
ops, over the state dict of effocr_amd.weights (timm >= 0.9 key names), written from the paper (Liu et al. 2021) and timm's semantics:
cyclic roll by -shift before and +shift after shifted-window attention, window partition / reverse, the region mask (-100 between
regions), the relative position index, patch merging in [x(2i,2j), x(2i+1,2j), x(2i,2j+1), x(2i+1,2j+1)] order, LayerNorm eps 1e-5.
The GPU tests compare the HIP encoder against it; tests/test_swin_host.py pins it to an independent implementation,
transformers' SwinModel.  It reads nothing outside the repository."""
import torch
import torch.nn.functional as F

from effocr_amd.weights import SWIN_CFG, strip_prefix

EPS = 1e-5


def _ln(x, w, b):
    return F.layer_norm(x, (x.shape[-1],), w, b, EPS)


def relative_index(ws):
    """[ws*ws, ws*ws] index into the (2ws-1)^2-row bias table: (dy + ws-1) * (2ws-1) + (dx + ws-1), d = coord(i) - coord(j)."""
    yy, xx = torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")
    y, x = yy.flatten(), xx.flatten()
    return (y[:, None] - y[None, :] + ws - 1) * (2 * ws - 1) + (x[:, None] - x[None, :] + ws - 1)


def windows(x, ws):
    """[B, H, W, C] -> [B * nW, ws*ws, C], windows row-major."""
    B, H, W, C = x.shape
    return x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def unwindows(w, ws, B, H, W):
    C = w.shape[-1]
    return w.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, C)


def region_mask(H, W, ws, shift, dtype):
    """[nW, ws*ws, ws*ws]: 0 within a region, -100 across (regions per axis of the rolled map: [0, n-ws), [n-ws, n-shift), [n-shift, n))."""
    def reg(n):
        r = torch.zeros(n, dtype=torch.long)
        r[n - ws:] = 1
        r[n - shift:] = 2
        return r
    ids = (reg(H)[:, None] * 3 + reg(W)[None, :]).to(dtype)
    w = windows(ids.view(1, H, W, 1), ws).squeeze(-1)          # [nW, ws*ws]
    d = w[:, None, :] - w[:, :, None]
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def window_attention(x, P, q, heads, ws, shift):
    """x [B, H, W, C] (already norm1'ed) -> [B, H, W, C] attention output before the residual."""
    B, H, W, C = x.shape
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    xw = windows(x, ws)                                        # [B nW, N, C]
    N, hd = ws * ws, C // heads
    qkv = F.linear(xw, P[q + "attn.qkv.weight"], P[q + "attn.qkv.bias"]).view(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    qq, kk, vv = qkv[0] * hd ** -0.5, qkv[1], qkv[2]
    attn = qq @ kk.transpose(-2, -1)                           # [B nW, heads, N, N]
    bias = P[q + "attn.relative_position_bias_table"][relative_index(ws).flatten()].view(N, N, heads).permute(2, 0, 1)
    attn = attn + bias[None]
    if shift:
        nW = (H // ws) * (W // ws)
        attn = (attn.view(B, nW, heads, N, N) + region_mask(H, W, ws, shift, attn.dtype)[None, :, None]).view(-1, heads, N, N)
    o = (attn.softmax(-1) @ vv).transpose(1, 2).reshape(-1, N, C)
    o = F.linear(o, P[q + "attn.proj.weight"], P[q + "attn.proj.bias"])
    o = unwindows(o, ws, B, H, W)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o


def patch_merge(x, P, p):
    x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1)
    return F.linear(_ln(x, P[p + "downsample.norm.weight"], P[p + "downsample.norm.bias"]), P[p + "downsample.reduction.weight"])


def swin_forward(arch, sd, x, tokens=False):
    """x [B,3,224,224] -> pooled features [B, 768] (dtype of x); tokens=True: the normed tokens [B, 49, 768] instead of their mean."""
    C0, depths, heads, ws = SWIN_CFG[arch]
    P = {k: v.to(x.dtype) for k, v in strip_prefix(sd).items()}
    h = F.conv2d(x, P["patch_embed.proj.weight"], P["patch_embed.proj.bias"], stride=4).permute(0, 2, 3, 1)
    h = _ln(h, P["patch_embed.norm.weight"], P["patch_embed.norm.bias"])
    for i, (nb, nh) in enumerate(zip(depths, heads)):
        p = f"layers.{i}."
        if i > 0:
            h = patch_merge(h, P, p)
        H = h.shape[1]
        w, sh = (H, 0) if H <= ws else (ws, ws // 2)             # timm: one window and no shift when the map fits a window
        for j in range(nb):
            q = p + f"blocks.{j}."
            h = h + window_attention(_ln(h, P[q + "norm1.weight"], P[q + "norm1.bias"]), P, q, nh, w, sh if j % 2 else 0)
            y = _ln(h, P[q + "norm2.weight"], P[q + "norm2.bias"])
            h = h + F.linear(F.gelu(F.linear(y, P[q + "mlp.fc1.weight"], P[q + "mlp.fc1.bias"])), P[q + "mlp.fc2.weight"], P[q + "mlp.fc2.bias"])
    h = _ln(h, P["norm.weight"], P["norm.bias"])
    B = h.shape[0]
    h = h.reshape(B, -1, h.shape[-1])
    return h if tokens else h.mean(dim=1)


def logits(arch, sd, x):
    """swin_forward + timm's classifier head (head.fc)."""
    P = strip_prefix(sd)
    f = swin_forward(arch, sd, x)
    return F.linear(f, P["head.fc.weight"].to(x.dtype), P["head.fc.bias"].to(x.dtype))


def hf_state_dict(sd):
    """timm key names -> transformers SwinModel key names (q / k / v split out of qkv; the patch merging of stage i > 0 is HF's
    downsample of stage i - 1; final norm -> layernorm)."""
    out = {}
    for k, v in strip_prefix(sd).items():
        if k.startswith("head."):
            continue
        if k.startswith("patch_embed."):
            out[k.replace("patch_embed.proj.", "embeddings.patch_embeddings.projection.").replace("patch_embed.norm.", "embeddings.norm.")] = v
            continue
        if k.startswith("norm."):
            out["layernorm." + k[len("norm."):]] = v
            continue
        parts = k.split(".")
        i = int(parts[1])
        if parts[2] == "downsample":
            out[f"encoder.layers.{i - 1}.downsample." + ".".join(parts[3:])] = v
            continue
        pre = f"encoder.layers.{i}.blocks.{parts[3]}."
        rest = ".".join(parts[4:])
        if rest.startswith("attn.qkv."):
            leaf = rest.rsplit(".", 1)[-1]
            for n, t in zip(("q_proj", "k_proj", "v_proj"), v.chunk(3, dim=0)):
                out[pre + f"attention.{n}.{leaf}"] = t.clone()
            continue
        rest = (rest.replace("attn.proj.", "attention.o_proj.")
                    .replace("attn.relative_position_bias_table", "attention.relative_position_bias.relative_position_bias_table")
                    .replace("norm1.", "layernorm_before.").replace("norm2.", "layernorm_after."))
        out[pre + rest] = v
    return out
