"""vit_small_patch8_224 / vit_base_patch8_224 on the MI355X (-m gpu): the streaming attention kernel alone against a float64 reference
(every token count around its tile sizes, exact padding, forced rescales), the 8x8 patch embedding alone, end-to-end parity with the
CPU restatement (tests/vit8_ref.py, pinned to transformers by tests/test_vit8_host.py) in every precision from 2 tokens to 785, batch /
position / chunk invariance, the fused normalise, the status word, the workspace, and the engines end to end.

Bounds.  End to end: the project's ViT bounds (tests/test_gpu_encoder.py), max norm AND worst-row relative L2.  The attention operator,
max norm relative to max|ref| on inputs already rounded to the mode's type: fp32 1e-5 (the exact-mode bound); 16-bit modes 2 x the error
of attention_emulated — the float64 computation with only the roundings csrc/vit8.hpp declares (P and the output) — on the same case,
computed on the CPU at run time; the factor 2 covers fp32 accumulation order and the hardware exp.  The patch embedding writes fp32 and
is compared on operands already rounded to the mode's type, so only fp32 accumulation over K = 192 is left: 1e-5 in every mode."""

import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.vit8_ref import attention_emulated, attention_ref, merge_heads, patch_embed, split_qkv, vit8_forward

pytestmark = pytest.mark.gpu

SMALL, BASE, TINY = "vit_small_patch8_224", "vit_base_patch8_224", "vit8_tiny_test"
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
PREC = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 8e-3}
OP_FP32 = 1e-5


def _header_tiles():
    """The kernel's tile sizes, read from csrc/vit8.hpp — the one place that states them: queries per workgroup (VIT8_QBLK), keys per tile
    in the 16-bit modes (VIT8_KTILE16) and in the fp32 mode (VIT8_KTILE32)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "effocr_amd", "csrc", "vit8.hpp")).read()
    return tuple(int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("VIT8_QBLK", "VIT8_KTILE16", "VIT8_KTILE32"))


TILES = _header_tiles()                                    # (128, 64, 32) as the header stands
# one token, one key pair, 33, 65, the patch-16 count 197 and the 785 of a 224^2 crop; and one below, at and one above every tile size,
# each of them in every precision
T_LIST = sorted({1, 2, 33, 65, 197, 785} | {t + d for t in TILES for d in (-1, 0, 1)})
B_OP, HEADS_OP = 2, 2


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


# -- the attention operator ---------------------------------------------------------------------------------------------------------
def _op_attn(dev, qkv, B, T, heads, tail=None):
    """effocr_vit8_op_attn on qkv [B*T, 3*heads*64] (its dtype picks the kernel); the output buffer is pre-filled with NaN.  ``tail``:
    rows that lie BEHIND the B*T rows in the same allocation — what a kernel that reads a padded key of the last crop would fetch."""
    L = _lib.vit8_lib()
    buf = qkv if tail is None else torch.cat([qkv, tail])
    buf = buf.to(dev).contiguous()
    out = torch.full((B * T, heads * 64), float("nan"), dtype=qkv.dtype, device=dev)
    _lib.vit8_check(L.effocr_vit8_op_attn(_lib.ptr(buf), B, T, heads, PREC[qkv.dtype], _lib.ptr(out), _lib.current_stream(dev)), "effocr_vit8_op_attn")
    torch.cuda.synchronize(dev)
    return out.cpu().double()


def _refs(qkv, B, T, heads, prec):
    """(float64 reference, bound) for one case: fp32 1e-5; 16-bit 2 x the emulation's own error."""
    q, k, v = split_qkv(qkv, B, T, heads)
    ref = merge_heads(attention_ref(q, k, v))
    if prec == "fp32":
        return ref, OP_FP32, 0.0
    emu = rel_err(merge_heads(attention_emulated(q, k, v, DT[prec])), ref)
    return ref, 2 * emu, emu


def _check_op(dev, what, qkv, B, T, heads, prec, tail=None):
    ref, bound, emu = _refs(qkv, B, T, heads, prec)
    got = _op_attn(dev, qkv, B, T, heads, tail)
    assert torch.isfinite(got).all()                       # every row was written
    e = rel_err(got, ref)
    print(f"vit8 op_attn {prec} T={T} {what}: max-norm {e:.3e}  emulated {emu:.3e}  bound {bound:.3e}")
    assert e <= bound
    return got, ref, bound


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("T", T_LIST)
def test_op_attention(dev, prec, T):
    g = torch.Generator().manual_seed(1000 + T)
    qkv = torch.randn(B_OP * T, 3 * HEADS_OP * 64, generator=g).to(DT[prec])
    _check_op(dev, "random", qkv, B_OP, T, HEADS_OP, prec)


def _padding_case(T, prec):
    """q = k = 0 and zero-mean v of distinct values: every output row is the mean of exactly that crop's T value rows.  The rows behind a
    crop in memory (the next crop's, and 64 rows of 50.0 behind the last) are what an unmasked padded key would bring in."""
    g = torch.Generator().manual_seed(2000 + T)
    qkv = torch.randn(B_OP * T, 3, HEADS_OP * 64, generator=g)
    qkv[:, :2] = 0
    qkv = qkv.view(B_OP * T, -1).to(DT[prec])
    tail = torch.full((64, 3 * HEADS_OP * 64), 50.0).to(DT[prec])
    return qkv, tail


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("T", T_LIST)
def test_op_attention_padding_is_exact(dev, prec, T):
    qkv, tail = _padding_case(T, prec)
    D = HEADS_OP * 64
    v = torch.cat([qkv, tail]).double()[:, 2 * D:]
    assert torch.unique(v[:B_OP * T], dim=0).shape[0] == B_OP * T                      # no two value rows are the same
    ref, bound, _ = _refs(qkv, B_OP, T, HEADS_OP, prec)
    mean = torch.stack([v[b * T:(b + 1) * T].mean(0) for b in range(B_OP)])
    assert rel_err(ref.view(B_OP, T, D), mean[:, None].expand(B_OP, T, D)) < 1e-13
    # on the CPU: a mean with one padded key included, or one live key dropped, is outside the bound at this T
    plus = torch.stack([v[b * T:(b + 1) * T + 1].mean(0) for b in range(B_OP)])
    assert rel_err(plus, mean) > bound, (rel_err(plus, mean), bound)
    if T > 1:
        minus = torch.stack([v[b * T:(b + 1) * T - 1].mean(0) for b in range(B_OP)])
        assert rel_err(minus, mean) > bound, (rel_err(minus, mean), bound)
    _check_op(dev, "q=k=0", qkv, B_OP, T, HEADS_OP, prec, tail)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("where", ["late", "early"])
def test_op_attention_forced_rescale(dev, prec, where):
    """One key scores +40 against every query, all others O(1).  late: it sits in the last key tile (key 780 of 785), so the running
    maximum jumps there and everything accumulated before is rescaled by e^-36; early: it sits in the first tile (key 3), so no later tile
    may raise the maximum.  The kernel rescales on every tile: there is no threshold to sweep."""
    T, spike = 785, {"late": 780, "early": 3}[where]
    D = HEADS_OP * 64
    g = torch.Generator().manual_seed(3000 + spike)
    qkv = torch.randn(B_OP * T, 3, HEADS_OP, 64, generator=g)
    qkv[:, 0, :, 0] = 4.0                                  # every query: 4 in dim 0 ...
    qkv[:, 1, :, 0] = 0.0                                  # ... which only the spiked key answers: 4 * 80 / 8 = +40
    for b in range(B_OP):
        qkv[b * T + spike, 1, :, 0] = 80.0
    qkv = qkv.view(B_OP * T, 3 * D).to(DT[prec])
    q, k, v = split_qkv(qkv.double(), B_OP, T, HEADS_OP)
    s = q @ k.transpose(-2, -1) / 8
    others = torch.cat([s[..., :spike], s[..., spike + 1:]], dim=-1)
    assert s[..., spike].min() > 34 and others.abs().max() < 6          # the plant: +40 (+- the O(1) rest) against O(1)
    got, ref, bound = _check_op(dev, f"{where} spike", qkv, B_OP, T, HEADS_OP, prec)
    # the spiked key's value row dominates: every output row of a crop is that row (the rest weighs e^-28 at most)
    vs = torch.stack([qkv[b * T + spike, 2 * D:].double() for b in range(B_OP)])[:, None].expand(B_OP, T, D).reshape(B_OP * T, D)
    e = rel_err(got, vs)
    print(f"vit8 op_attn {prec} T={T} {where} spike: distance from the spiked value row {e:.3e}")
    assert e <= bound + T * float(np.exp(-28.0))           # (+ what the other keys can weigh at most: the reference holds it, the row does not)


# -- the patch embedding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img,B,D", [(8, 1, 128), (8, 3, 128), (24, 1, 128), (24, 3, 384), (224, 1, 128), (224, 3, 128)])
def test_op_patch_embed(dev, prec, img, B, D):
    g = torch.Generator().manual_seed(img + B)
    T = (img // 8) ** 2 + 1
    x = _crops(B, img, img + B).to(DT[prec]).float()       # operands already in the mode's type: the reference sees the same values
    w = (torch.randn(D, 3, 8, 8, generator=g) / 192 ** 0.5).to(DT[prec])
    bias, cls, pos = torch.randn(D, generator=g) * 0.1, torch.randn(1, 1, D, generator=g) * 0.5, torch.randn(1, T, D, generator=g) * 0.5
    ref = patch_embed(x.double(), w.double(), bias.double(), cls.double(), pos.double()).reshape(B * T, D)
    L = _lib.vit8_lib()
    xd, wd, bd, pd = x.to(dev), w.reshape(D, 192).contiguous().to(dev), bias.to(dev), pos.reshape(T, D).contiguous().to(dev)
    c0 = (cls.reshape(D) + pos[0, 0]).to(dev)
    col = torch.empty(B * (T - 1) * 192, dtype=DT[prec], device=dev)
    out = torch.full((B * T, D), float("nan"), device=dev)
    _lib.vit8_check(L.effocr_vit8_op_patch_embed(_lib.ptr(xd), B, img, D, PREC[DT[prec]], _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(c0), _lib.ptr(pd),
                                                 _lib.ptr(col), _lib.ptr(out), _lib.current_stream(dev)), "effocr_vit8_op_patch_embed")
    torch.cuda.synchronize(dev)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    e = rel_err(got, ref)
    print(f"vit8 op_patch_embed {prec} img {img} B={B} D={D}: max-norm {e:.3e}")
    assert e <= 1e-5
    assert torch.equal(out.cpu()[::T], c0.cpu()[None].expand(B, D))        # the cls rows are cls + pos[0], bit for bit


# -- end to end ---------------------------------------------------------------------------------------------------------------------
def _crops(B, img, seed):
    """ImageNet-normalised-looking crops: noise plus, per crop, a few bright / dark strokes at positions of its own (a different
    glyph per crop), some of them across patch borders."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, img, img, generator=g) * 0.5
    for b in range(B):
        for _ in range(4):
            y0, x0 = (int(v) for v in torch.randint(0, max(img - 6, 1), (2,), generator=g))
            h, w = (int(v) for v in torch.randint(3, max(img // 2, 4), (2,), generator=g))
            x[b, :, y0:y0 + h, x0:x0 + w] += float(torch.randn(1, generator=g)) * 2.5
    return x


def _engine(arch, sd, img, prec, dev):
    from effocr_amd.encoders import make_encoder
    return make_encoder(arch, sd, img_size=img, precision=prec, device=dev)


_REFS = {}


def _ref(arch, img, scale, n, dtype):
    """(state dict, n crops, their restatement embeddings in ``dtype``), computed once per case and shared by the precisions and batch
    sizes (the restatement computes a crop from that crop alone, so a batch of B is the first B rows)."""
    key = (arch, img, scale)
    if key not in _REFS:
        sd, x = W.init_state_dict(arch, seed=1, img_size=img, scale=scale), _crops(n, img, 7 + img)
        with torch.no_grad():
            _REFS[key] = (sd, x, vit8_forward(sd, x.to(dtype)).float())
    return _REFS[key]


def _check_parity(dev, arch, img, scale, B, prec, n, dtype):
    sd, x, ref = _ref(arch, img, scale, n, dtype)
    if n > 1:
        # on the reference alone: two crops' embeddings differ by 10 x the bound at least, so a forward that ignores its input cannot pass
        apart = min(((ref[i] - ref[j]).abs().max() / ref.abs().max()).item() for i in range(n) for j in range(i))
        assert apart >= 10 * REL[prec], apart
    x, ref = x[:B], ref[:B]
    enc = _engine(arch, sd, img, prec, dev)
    assert enc.call_size_invariant is True
    got = enc.forward(x.to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    print(f"vit8 {arch} img {img} {prec} {scale} B={B}: max-norm {e_max:.2e}, row L2 {e_row:.2e}")
    assert e_max <= REL[prec] and e_row <= REL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("scale", ["unit", "trained"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("img", [8, 48, 72, 224])          # 2, 37, 82 and 785 tokens: one key tile, two, and 13 with one live key in the last
def test_parity_tiny(dev, prec, scale, B, img):
    _check_parity(dev, TINY, img, scale, B, prec, 3, torch.float64)


@pytest.mark.parametrize("arch,B,prec", [(SMALL, 2, "fp32"), (SMALL, 2, "fp16"), (SMALL, 2, "bf16"), (BASE, 1, "fp16")])
def test_parity_full(dev, arch, B, prec):
    """The real widths at 224^2 (785 tokens, 12 blocks), trained magnitudes, against the restatement in float32."""
    _check_parity(dev, arch, 224, "trained", B, prec, B, torch.float32)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img", [72, 224])
def test_batch_position_and_chunk_invariance(dev, prec, img):
    enc = _engine(TINY, W.init_state_dict(TINY, seed=2, img_size=img), img, prec, dev)
    crop = _crops(1, img, 21).to(dev)
    alone = enc.forward(crop)
    five = _crops(5, img, 22).to(dev)
    for at in (0, 4):
        call = five.clone()
        call[at] = crop[0]
        assert torch.equal(enc.forward(call)[at:at + 1], alone), at
    big = _crops(70, img, 23).to(dev)
    big[41] = crop[0]
    assert torch.equal(enc.forward(big)[41:42], alone)
    whole = enc.forward(five)
    for chunk in (1, 3, 0):
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(crop), alone), chunk
        assert torch.equal(enc.forward(five), whole), chunk
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_l2_normalize_fused(dev, prec):
    enc = _engine(TINY, W.init_state_dict(TINY, seed=4, img_size=64), 64, prec, dev)
    x = _crops(4, 64, 3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    torch.testing.assert_close(nrm, F.normalize(raw, dim=1), rtol=0, atol=2e-7)
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_status_reports_nonfinite_input(dev, prec):
    enc = _engine(TINY, W.init_state_dict(TINY, seed=5, img_size=64), 64, prec, dev)
    x = _crops(4, 64, 8).to(dev)
    enc.forward(x)
    enc.check_status()
    x[2, 1, 10, 10] = float("nan")
    emb = enc.forward(x)
    with pytest.raises(_lib.EffOCRHipError, match="code -6"):
        enc.check_status()
    assert not torch.isfinite(emb[2]).all()
    assert torch.isfinite(emb[[0, 1, 3]]).all()            # the other crops of the call are untouched
    enc.check_status()                                     # read-and-clear
    enc.forward(x)
    enc.reset_status()                                     # cleared without being read
    enc.check_status()


def test_workspace_is_honoured_and_too_small_is_refused(dev):
    img, B = 64, 3
    enc = _engine(TINY, W.init_state_dict(TINY, seed=6, img_size=img), img, "fp16", dev)
    L = enc._L
    need = enc.workspace_bytes(B)
    x = _crops(B, img, 1).to(dev)
    emb = torch.empty(B, 128, device=dev)
    # the forward stays inside the bytes it asked for: a guard band behind them is untouched
    guard = 4096
    ws = torch.zeros(need + guard, dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    s = _lib.current_stream(dev)
    assert L.effocr_vit8_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    assert b"workspace" in L.effocr_vit8_last_error()
    assert L.effocr_vit8_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.all(ws[need:] == 0xA5)
    assert torch.equal(emb, enc.forward(x))
    with pytest.raises(ValueError):
        enc.forward(x.half())                              # fp32 crops only


def test_end_to_end_engines(dev, tmp_path):
    """A saved vit8_tiny_test checkpoint (64^2 crops, 65 tokens) through AutoEncoderFactory.load, EffRecognizer (architecture and crop
    size inferred), the Recognizer pipeline over an index of planted glyph embeddings, and the classifier."""
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory, Vit8Encoder
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    n, ncls, img = 8, 7, 64
    sd = W.init_state_dict(TINY, seed=7, img_size=img, num_classes=ncls)
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    glyphs = _crops(n, img, 31)
    q = glyphs + 0.05 * torch.randn(glyphs.shape, generator=torch.Generator().manual_seed(32))
    want = torch.arange(n) + 250
    chars = [chr(0x4E00 + i) for i in range(500 + n)]
    dis = F.normalize(torch.randn(500, 128, generator=torch.Generator().manual_seed(9)), dim=1)

    ids = {}
    for prec in ("fp32", "fp16"):
        er = EffRecognizer(str(ckpt), precision=prec, device=dev)
        assert er.arch == TINY and er.img_size == img and er.crop_dtype == torch.float32 and er.call_size_invariant
        if prec == "fp32":                                 # the index holds the glyphs' fp32 embeddings among 500 distractors
            planted = torch.from_numpy(er.run(glyphs.numpy())[0])
            cos = F.normalize(planted, dim=1) @ F.normalize(planted, dim=1).T
            assert (cos - 2 * torch.eye(n)).max() < 0.99   # the glyphs are told apart
            index = torch.cat([dis[:250], F.normalize(planted, dim=1), dis[250:]])
        emb = er.run(q.numpy())[0]
        assert emb.shape == (n, 128) and emb.dtype == np.float32
        ids[prec] = (F.normalize(torch.from_numpy(emb), dim=1) @ index.T).argmax(dim=1)
        assert torch.equal(ids[prec], want)

    enc = AutoEncoderFactory("timm", TINY, img_size=img).load(str(ckpt))
    enc.to(dev).eval()
    assert isinstance(enc.engine, Vit8Encoder)
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, chars, knn=10)
    _, _, text = rec(q.to(dev))
    assert text == "".join(chars[i] for i in want.tolist())

    clf = AutoClassifierFactory("timm", TINY, n_classes=ncls, img_size=img).load(str(ckpt))
    clf.to(dev).eval()
    lg = clf(q.to(dev))
    assert lg.shape == (n, ncls)
    want_lg = F.linear(clf.embed(q.to(dev)).cpu(), sd["head.weight"], sd["head.bias"])     # the CPU head on the device's embeddings
    torch.testing.assert_close(lg.cpu(), want_lg, rtol=1e-4, atol=1e-4)
    assert torch.equal(clf.predict(q.to(dev)), lg.argmax(dim=1))
    clf.check_status()
