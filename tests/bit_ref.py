"""BiT ResNetV2 (resnetv2_50x1_bitm / resnetv2_101x1_bitm) restated in torch functional ops over timm's keys, in the dtype of its input
(float64 for the references), a rounding-emulating form of it, float64 restatements of libeffocr_bit.so's three operators, and those
operators' test data, derived error bounds and mutants (tests/test_bit_host.py, tests/test_gpu_bit_ops.py, tests/test_gpu_bit.py).

The network restatement is pinned against ``transformers.BitModel`` by tests/test_bit_host.py through BIT_HF_KEYS.
"""
import torch
import torch.nn.functional as F

from effocr_amd.weights import BIT_CFG, strip_prefix

GROUPS, GN_EPS, WS_EPS = 32, 1e-5, 1e-8
DTYPES = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
# unit round-offs (half an ulp, relative) of the three operand types
U = {"fp32": 2.0 ** -24, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
# half the spacing of the smallest subnormals: what a rounding can cost where the relative bound has gone to zero
TINY = {"fp32": 2.0 ** -150, "fp16": 2.0 ** -25, "bf16": 2.0 ** -134}


def hf_key(k):
    """timm key -> transformers.BitModel key (a bijection on the encoder's parameters)."""
    if k == "stem.conv.weight":
        return "embedder.convolution.weight"
    if k.startswith("stages."):
        _, i, _, j, rest = k.split(".", 4)
        return f"encoder.stages.{i}.layers.{j}.{rest}"
    return k


def standardize(w):
    """timm StdConv2d: per output channel, (w - mean) / sqrt(biased var + 1e-8) over Cin x KH x KW."""
    mu = w.mean(dim=(1, 2, 3), keepdim=True)
    var = w.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
    return (w - mu) / torch.sqrt(var + WS_EPS)


def _rnd(x, dt):
    return x if dt is None else x.to(dt).to(x.dtype)


def bit_forward(arch, sd, x, round_to=None):
    """[B, 3, S, S] -> [B, 2048] pooled features in x's dtype.  ``round_to`` (a torch dtype) emulates the library's 16-bit (or fp32) modes
    with exact accumulation: the standardised weights, the crop, every convolution's output after its residual add and every
    GroupNorm + ReLU output are rounded to it; the head stays unrounded, as the library's does."""
    sd = strip_prefix(sd)
    dt = x.dtype
    Wt = {k: (_rnd(standardize(v.to(dt)), round_to) if v.dim() == 4 else v.to(dt)) for k, v in sd.items() if not k.startswith("head.")}

    def gn(t, p):
        return _rnd(F.relu(F.group_norm(t, GROUPS, Wt[p + ".weight"], Wt[p + ".bias"], GN_EPS)), round_to)

    x = _rnd(x, round_to)
    x = _rnd(F.conv2d(x, Wt["stem.conv.weight"], stride=2, padding=3), round_to)
    x = F.max_pool2d(F.pad(x, (1, 1, 1, 1), value=0.0), 3, 2)
    for si, depth in enumerate(BIT_CFG[arch]):
        for bi in range(depth):
            p = f"stages.{si}.blocks.{bi}."
            stride = 2 if (bi == 0 and si > 0) else 1
            pre = gn(x, p + "norm1")
            sc = x
            if bi == 0:
                sc = _rnd(F.conv2d(pre, Wt[p + "downsample.conv.weight"], stride=stride), round_to)
            y = _rnd(F.conv2d(pre, Wt[p + "conv1.weight"]), round_to)
            y = _rnd(F.conv2d(gn(y, p + "norm2"), Wt[p + "conv2.weight"], stride=stride, padding=1), round_to)
            x = _rnd(F.conv2d(gn(y, p + "norm3"), Wt[p + "conv3.weight"]) + sc, round_to)
    x = F.relu(F.group_norm(x, GROUPS, Wt["norm.weight"], Wt["norm.bias"], GN_EPS))
    return x.mean(dim=(2, 3))


def bit_logits(arch, sd, x):
    """timm's classifier on the pooled features: the 1x1-conv head.fc as a matrix."""
    sd = strip_prefix(sd)
    w = sd["head.fc.weight"].to(x.dtype)
    return bit_forward(arch, sd, x) @ w.reshape(w.shape[0], -1).T + sd["head.fc.bias"].to(x.dtype)


# ----------------------------------------------------------------------------------------------------------------- operators (NHWC)
def _stats(x, unbiased=False):
    """x [B, HW, C] -> per (crop, group) mean and variance, shaped to broadcast over [B, HW, 32, cpg]."""
    B, HW, C = x.shape
    g = x.reshape(B, HW, GROUPS, C // GROUPS)
    return g, g.mean(dim=(1, 3), keepdim=True), g.var(dim=(1, 3), unbiased=unbiased, keepdim=True)


def gn_relu_ref(x, gamma, beta):
    """relu(GroupNorm_32(x) * gamma + beta) on NHWC [B, HW, C], in x's dtype."""
    g, mu, var = _stats(x)
    xh = ((g - mu) / torch.sqrt(var + GN_EPS)).reshape(x.shape)
    return F.relu(xh * gamma + beta)


def gn_relu_emul(x, gamma, beta, prec):
    """The kernel's contract on the CPU: float32 statistics from deviations about a shift (the group's first channel at the crop's first
    pixel), per tile of max(1, 16384 / C) pixels as (mean, M2) about the tile's own mean and merged by Chan's formula in tile order,
    float32 apply, one rounding to ``prec``; returned as float64."""
    B, HW, C = x.shape
    cpg = C // GROUPS
    g = x.float().reshape(B, HW, GROUPS, cpg)
    d = g - g[:, :1, :, :1]
    tp = max(1, 16384 // C)
    n = torch.zeros((), dtype=torch.float32)
    mu = torch.zeros(B, 1, GROUPS, 1)
    m2 = torch.zeros(B, 1, GROUPS, 1)
    for p0 in range(0, HW, tp):
        t = d[:, p0:p0 + tp]
        nb = torch.tensor(float(t.shape[1] * cpg))
        mb = t.mean(dim=(1, 3), keepdim=True)
        m2b = ((t - mb) ** 2).sum(dim=(1, 3), keepdim=True)
        nt, dl = n + nb, mb - mu
        mu = mu + dl * (nb / nt)
        m2 = m2 + m2b + dl * dl * (n * nb / nt)
        n = nt
    var = m2 / n
    y = ((d - mu) * (1.0 / torch.sqrt(var + GN_EPS))).reshape(x.shape) * gamma.float() + beta.float()
    return F.relu(y).to(DTYPES[prec]).double()


def gn_xhat(x):
    """The normalised values themselves (what the bound scales with)."""
    g, mu, var = _stats(x)
    return ((g - mu) / torch.sqrt(var + GN_EPS)).reshape(x.shape)


def gn_bound(x, gamma, beta, prec):
    """Element-wise bound on |kernel - float64 reference| for an output rounded once to ``prec``, statistics and arithmetic in fp32.

    With y = x^ gamma + beta: (a) the output rounding costs U[prec] (|y| + b) + TINY; (b) the fp32 budget b = K u32 (|gamma| (|x^| + 1) +
    |beta|).  The mean and M2 are sums of deviations about a shift, so their rounding errors are relative to the deviations: a chain of at
    most 8 + 64 additions per tile and one Chan merge per tile (at most 49 tiles here), random-walk ~ sqrt(121) = 11 roundings, moves
    the mean by about 11 u32 sigma (the "+ 1") and 1/sigma by 11 u32 relative (the |x^| term); the apply is 4 more roundings of
    the products.  K = 16 covers both."""
    u32 = U["fp32"]
    xh = gn_xhat(x)
    y = xh * gamma + beta
    b = 16 * u32 * (gamma.abs() * (xh.abs() + 1) + beta.abs())
    return U[prec] * (F.relu(y) + b) + b + TINY[prec]


def gn_mutants(x, gamma, beta):
    """{name: wrong output} — what the bound must reject (float64, on the same inputs)."""
    B, HW, C = x.shape
    cpg = C // GROUPS
    g, mu, var = _stats(x)
    out = {}

    def fin(gh):
        return gh.reshape(x.shape) * gamma + beta
    out["unbiased variance"] = F.relu(fin((g - mu) / torch.sqrt(_stats(x, True)[2] + GN_EPS)))
    out["eps omitted"] = F.relu(fin((g - mu) / torch.sqrt(var)))
    # group = c mod 32: channels interleaved
    gi = x.reshape(B, HW, cpg, GROUPS)
    mi, vi = gi.mean(dim=(1, 2), keepdim=True), gi.var(dim=(1, 2), unbiased=False, keepdim=True)
    out["group = c mod 32"] = F.relu(fin(((gi - mi) / torch.sqrt(vi + GN_EPS))))
    xh = ((g - mu) / torch.sqrt(var + GN_EPS))
    out["gamma / beta indexed by group"] = F.relu(xh * gamma[:GROUPS].reshape(1, 1, GROUPS, 1) + beta[:GROUPS].reshape(1, 1, GROUPS, 1)).reshape(x.shape)
    if B > 1:
        out["statistics of the neighbouring crop"] = F.relu(fin((g - mu.roll(1, 0)) / torch.sqrt(var.roll(1, 0) + GN_EPS)))
    out["ReLU omitted"] = fin(xh)
    return out


def gn_mutant_ex2(x, gamma, beta):
    """E[x^2] - mean^2 with float32 statistics: the form the kernel must not use (rejected on the mean = 20 sigma case)."""
    B, HW, C = x.shape
    g = x.float().reshape(B, HW, GROUPS, C // GROUPS)
    mu = g.mean(dim=(1, 3), keepdim=True)
    var = (g * g).mean(dim=(1, 3), keepdim=True) - mu * mu
    xh = ((g - mu) / torch.sqrt(var + GN_EPS)).double().reshape(x.shape)
    return F.relu(xh * gamma + beta)


# GroupNorm cases: name -> (B, HW, C, mean in sigmas, scale, precisions)
GN_CASES = {
    "head width, one pixel": (3, 1, 2048, 0.0, 1.0, ("fp32", "fp16", "bf16")),
    "two channels per group": (2, 64, 64, 0.0, 1.0, ("fp32", "fp16", "bf16")),
    "odd pixel count": (2, 49, 256, 0.0, 1.0, ("fp32", "fp16", "bf16")),
    "49 tiles": (1, 3136, 256, 0.0, 1.0, ("fp32", "fp16", "bf16")),
    "mean = 20 sigma": (2, 200, 128, 20.0, 1.0, ("fp32",)),
    "scaled by 3e-3": (2, 100, 64, 0.0, 3e-3, ("fp32",)),
}


def gn_case(name, prec):
    """(x [B, HW, C], gamma, beta) float64, x already rounded to ``prec``.  Every crop and every group has its own offset and scale, so
    that statistics taken from the wrong crop or the wrong channels show."""
    B, HW, C, mean, scale, _ = GN_CASES[name]
    g = torch.Generator().manual_seed(1000 + len(name) + B * 7 + HW)
    x = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    grp = torch.rand(B, 1, GROUPS, 1, generator=g, dtype=torch.float64) + 0.5          # per (crop, group) sigma
    off = torch.randn(B, 1, GROUPS, 1, generator=g, dtype=torch.float64) * 0.5 + mean  # ... and mean, in sigmas
    ch = torch.randn(1, 1, C, generator=g, dtype=torch.float64) * 0.3                  # a per-channel offset within the group
    x = ((x + ch).reshape(B, HW, GROUPS, C // GROUPS) * grp + off * grp).reshape(B, HW, C) * scale
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    return x.to(DTYPES[prec]).double(), gamma.float().double(), beta.float().double()


def stem_pool_ref(x):
    """max_pool2d(pad(x, 1, value 0), 3, 2) on NHWC [B, H, W, C]."""
    y = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=0.0), 3, 2)
    return y.permute(0, 2, 3, 1).contiguous()


def stem_pool_mutant(x):
    """-inf padding (max_pool2d's own padding=1): differs wherever a border window is all negative."""
    return F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, padding=1).permute(0, 2, 3, 1).contiguous()


POOL_CASES = {"16^2": (2, 16, 64), "112^2": (1, 112, 64)}


def pool_case(name, prec):
    """x [B, S, S, C] float64 rounded to ``prec``, with negative rows and columns at the borders (where the zero padding wins)."""
    B, S, C = POOL_CASES[name]
    g = torch.Generator().manual_seed(77 + S)
    x = torch.randn(B, S, S, C, generator=g, dtype=torch.float64)
    x[:, :2] = -x[:, :2].abs() - 0.1
    x[:, :, :2] = -x[:, :, :2].abs() - 0.1
    x[:, -2:] = -x[:, -2:].abs() - 0.1
    return x.to(DTYPES[prec]).double()


def head_ref(x, gamma, beta, l2):
    """mean over HW of relu(GroupNorm_32(x) * gamma + beta) on NHWC [B, HW, C] (+ F.normalize)."""
    e = gn_relu_ref(x, gamma, beta).mean(dim=1)
    return F.normalize(e, dim=1) if l2 else e


def head_bound(x, gamma, beta, l2):
    """Element-wise bound on |kernel - float64 reference|: the head is fp32 throughout, so it is the GroupNorm fp32 budget averaged over
    the pixels plus the fp32 mean's own roundings (HW additions, bounded by HW u32 of the mean of |y|); normalising divides both the value
    and its error by the row norm and adds the norm's own relative error (bounded by the same budget relative to the norm)."""
    u32 = U["fp32"]
    xh = gn_xhat(x)
    y = F.relu(xh * gamma + beta)
    b = (16 * u32 * (gamma.abs() * (xh.abs() + 1) + beta.abs())).mean(dim=1) + (x.shape[1] + 2) * u32 * y.mean(dim=1)
    if not l2:
        return b + 1e-45
    e = y.mean(dim=1)
    nrm = e.norm(dim=1, keepdim=True)
    return b / nrm + (e.abs() / nrm) * (b.norm(dim=1, keepdim=True) / nrm + 4 * u32) + 1e-45


def head_mutants(x, gamma, beta, l2):
    g, mu, var = _stats(x)
    xh = ((g - mu) / torch.sqrt(var + GN_EPS)).reshape(x.shape)
    out = {"mean before ReLU": F.relu((xh * gamma + beta).mean(dim=1))}
    if l2:
        out["mean before ReLU"] = F.normalize(out["mean before ReLU"], dim=1)
        out["normalise omitted"] = head_ref(x, gamma, beta, False)
    return out


HEAD_CASES = {"HW 1": (3, 1, 2048), "HW 4": (2, 4, 2048), "HW 49": (2, 49, 2048)}


def head_case(name, prec):
    B, HW, C = HEAD_CASES[name]
    g = torch.Generator().manual_seed(500 + HW)
    x = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    grp = torch.rand(B, 1, GROUPS, 1, generator=g, dtype=torch.float64) + 0.5
    off = torch.randn(B, 1, GROUPS, 1, generator=g, dtype=torch.float64)
    x = (x.reshape(B, HW, GROUPS, C // GROUPS) * grp + off).reshape(B, HW, C)
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64) * 0.2
    return x.to(DTYPES[prec]).double(), gamma.float().double(), beta.float().double()


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound: accepted when <= 1."""
    return ((got - ref).abs() / bound).max().item()


def crops(B, seed, img):
    """Normalised-looking crops with bright / dark strokes near the borders, asymmetric so that a transposed crop differs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, img, img, generator=g) * 0.5
    s = max(img // 32, 1)
    for b in range(B):
        o = int(torch.randint(0, s + 1, (1,), generator=g))
        x[b, :, 1 + o:4 * s + o, 0:2 * s] += 2.5
        x[b, :, img - 4 * s:img, img - 3 * s - o:img - o] -= 2.0
        x[b, :, img // 2:img // 2 + s, :] += 1.5
    return x
