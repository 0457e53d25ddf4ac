"""beit_base_patch16_224 / beitv2_base_patch16_224 on the MI355X (-m gpu): the bias-attention kernels alone against a float64
restatement, end-to-end parity with the CPU restatement (tests/beit_ref.py, pinned to transformers by tests/test_beit_host.py) in every
precision from one patch to 196, batch / position / chunk invariance, the fused normalise, the status word, the workspace, and the
engines end to end."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from effocr_amd import _lib
from effocr_amd import weights as W
from tests.beit_ref import beit_forward, bias_attention

pytestmark = pytest.mark.gpu

ARCH, TINY = "beit_base_patch16_224", "beit_tiny_test"
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}

# End-to-end bounds, max norm AND worst-row relative L2: fp32 = the exact mode; fp16 = north_star's 1e-3; bf16 has no project-wide
# number (ViT uses 8e-3 and Swin 1e-2, each measured): BF16_MEASURED is the worst case over the cases of test_parity_tiny and
# test_parity_base (beit_tiny_test, 16^2, trained magnitudes, B = 1, max norm; profiles/beit_parity.txt), the bound 1.5 x that = 4.29e-3.
# fp16's worst case in the same run is 4.91e-4, fp32's 1.25e-6.
BF16_MEASURED = 2.86e-3
REL = {"fp32": 1e-5, "fp16": 1e-3, "bf16": 1.5 * BF16_MEASURED}
# The lone attention operator in the 16-bit modes, against the float64 restatement on the SAME rounded inputs, max norm: there is no
# project number, so OP_MEASURED is the worst case over test_op_attention's cases (profiles/beit_parity.txt) and the bound 1.5 x that
# for seed-to-seed spread: fp16 3.86e-4 -> 5.79e-4, bf16 3.43e-3 -> 5.15e-3 (both at W = 1, random q and k; fp32's worst is 1.23e-6).
# What is left in that error: P and the output rounded to the 16-bit type (half an ulp is 2^-12 / 2^-9 of the value), fp32 accumulation.
OP_MEASURED = {"fp16": 3.86e-4, "bf16": 3.43e-3}
OP_REL = {"fp32": 1e-5, "fp16": 1.5 * OP_MEASURED["fp16"], "bf16": 1.5 * OP_MEASURED["bf16"]}


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def row_l2_err(got, ref):
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


# -- the attention operator ---------------------------------------------------------------------------------------------------------
def _op_attn(dev, qkv, table, B, Wn, heads):
    """effocr_beit_op_attn on qkv [B*T, 3*heads*64] (its dtype picks the kernel) and table [(2 Wn - 1)^2 + 3, heads] fp32."""
    L = _lib.beit_lib()
    prec = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}[qkv.dtype]
    q, t = qkv.to(dev).contiguous(), table.to(dev, torch.float32).contiguous()
    out = torch.full((q.shape[0], heads * 64), float("nan"), dtype=qkv.dtype, device=dev)
    _lib.beit_check(L.effocr_beit_op_attn(_lib.ptr(q), _lib.ptr(t), B, Wn, heads, prec, _lib.ptr(out), _lib.current_stream(dev)), "effocr_beit_op_attn")
    torch.cuda.synchronize(dev)
    return out.cpu()


def _op_ref(qkv, table, B, Wn, heads):
    T = Wn * Wn + 1
    q, k, v = qkv.double().view(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return bias_attention(q, k, v, table.double(), Wn).transpose(1, 2).reshape(B * T, heads * 64)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("Wn", [1, 2, 4, 8, 14])           # T = 2, 5, 17, 65, 197: one patch; under one query block; one key in a third
@pytest.mark.parametrize("zero_qk", [False, True])         # key tile; the full 7 tiles with 5 live keys in the last
def test_op_attention(dev, prec, Wn, zero_qk):
    B, heads, T = 3, 2, Wn * Wn + 1
    g = torch.Generator().manual_seed(100 * Wn + zero_qk)
    qkv = torch.randn(B * T, 3 * heads * 64, generator=g)
    table = torch.randn((2 * Wn - 1) ** 2 + 3, heads, generator=g)
    if zero_qk:
        # q = k = 0 and a table of distinct values N(0, 3): the output is exactly softmax(bias row) . V — an index error shows at full size
        qkv.view(B * T, 3, heads * 64)[:, :2] = 0
        table = table * 3
        assert table.flatten().unique().numel() == table.numel()
    qkv = qkv.to(DT[prec])
    got = _op_attn(dev, qkv, table, B, Wn, heads).double()
    ref = _op_ref(qkv, table, B, Wn, heads)
    assert torch.isfinite(got).all()                       # every row was written
    e = rel_err(got, ref)
    print(f"beit op_attn {prec} W={Wn} T={T} {'q=k=0' if zero_qk else 'random'}: max-norm {e:.2e}")
    assert e <= OP_REL[prec]


# -- end to end ---------------------------------------------------------------------------------------------------------------------
def _sd(arch, img, seed, trained=False, num_classes=0):
    if not trained:
        return W.init_state_dict(arch, seed=seed, img_size=img, num_classes=num_classes)
    # trained magnitudes: timm's own init (std 0.02 linears, identity LayerNorms, layer scale 0.1, biases N(0, 0.02)) with bias tables
    # of a trained model's size, N(0, 1)
    sd = W.init_state_dict(arch, seed=seed, img_size=img, scale="timm", num_classes=num_classes)
    g = torch.Generator().manual_seed(seed + 100)
    for k in sd:
        if k.endswith("relative_position_bias_table"):
            sd[k] = torch.randn(sd[k].shape, generator=g)
    return sd


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


def _ref(arch, img, trained, n):
    """(state dict, n crops, their float64 restatement embeddings), computed once per case and shared by the precisions and batch sizes
    (the restatement computes a crop from that crop alone, so a batch of B is the first B rows).  Parity against it means something
    only if it tells crops apart: every pair of its embeddings has cosine < 0.99."""
    key = (arch, img, trained)
    if key not in _REFS:
        sd, x = _sd(arch, img, 1, trained), _crops(n, img, 7 + img)
        ref = beit_forward(arch, sd, x.double()).float()
        cos = F.normalize(ref, dim=1) @ F.normalize(ref, dim=1).T
        worst = (cos - 2 * torch.eye(n)).max().item()
        print(f"beit reference {arch} img {img} {'trained' if trained else 'unit'}: largest cosine between two crops {worst:.3f}")
        assert worst < 0.99
        _REFS[key] = (sd, x, ref)
    return _REFS[key]


def _check_parity(dev, arch, img, trained, B, prec, n):
    sd, x, ref = _ref(arch, img, trained, n)
    x, ref = x[:B], ref[:B]
    enc = _engine(arch, sd, img, prec, dev)
    assert enc.call_size_invariant is True
    got = enc.forward(x.to(dev)).cpu()
    enc.check_status()
    e_max, e_row = rel_err(got, ref), row_l2_err(got, ref)
    print(f"beit {arch} img {img} {prec} {'trained' if trained else 'unit'} B={B}: max-norm {e_max:.2e}, row L2 {e_row:.2e}")
    assert e_max <= REL[prec] and e_row <= REL[prec]


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("trained", [False, True])
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("img", [16, 64, 128, 224])        # GEMM rows B T from 2 to 985, a tile multiple only by accident
def test_parity_tiny(dev, prec, trained, B, img):
    _check_parity(dev, TINY, img, trained, B, prec, 5)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("trained", [False, True])
def test_parity_base(dev, prec, trained):
    _check_parity(dev, ARCH, 224, trained, 2, prec, 2)


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("img", [64, 224])
def test_batch_position_and_chunk_invariance(dev, prec, img):
    enc = _engine(TINY, _sd(TINY, img, 2), img, prec, dev)
    x7 = _crops(7, img, 21).to(dev)
    base = enc.forward(x7)
    singles = torch.cat([enc.forward(x7[i:i + 1]) for i in range(7)])
    assert torch.equal(singles, base)
    n = 40
    big = _crops(n, img, 140).to(dev)
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(n))[:7].to(dev)
    big[pos] = x7
    assert torch.equal(enc.forward(big)[pos], base)
    for chunk in (5, 3, 1, 0):
        enc.set_chunk(chunk)
        assert torch.equal(enc.forward(x7), base), chunk
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_l2_normalize_fused(dev, prec):
    enc = _engine(TINY, _sd(TINY, 64, 4), 64, prec, dev)
    x = _crops(4, 64, 3).to(dev)
    raw = enc.forward(x)
    nrm = enc.forward(x, normalize=True)
    torch.testing.assert_close(nrm, F.normalize(raw, dim=1), rtol=0, atol=2e-7)
    enc.check_status()


@pytest.mark.parametrize("prec", ["fp16", "bf16", "fp32"])
def test_status_reports_nonfinite_input(dev, prec):
    enc = _engine(TINY, _sd(TINY, 64, 5), 64, prec, dev)
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
    enc = _engine(TINY, _sd(TINY, img, 6), img, "fp16", dev)
    L = enc._L
    need = enc.workspace_bytes(B)
    x = _crops(B, img, 1).to(dev)
    emb = torch.empty(B, 128, device=dev)
    # the forward stays inside the bytes it asked for: a guard band behind them is untouched
    guard = 4096
    ws = torch.zeros(need + guard, dtype=torch.uint8, device=dev)
    ws[need:] = 0xA5
    s = _lib.current_stream(dev)
    assert L.effocr_beit_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need - 1, s) == -3
    assert b"workspace" in L.effocr_beit_last_error()
    assert L.effocr_beit_forward(enc._h, _lib.ptr(x), B, _lib.ptr(emb), 0, _lib.ptr(ws), need, s) == 0
    torch.cuda.synchronize(dev)
    assert torch.all(ws[need:] == 0xA5)
    assert torch.equal(emb, enc.forward(x))
    with pytest.raises(ValueError):
        enc.forward(x.half())                              # fp32 crops only


def test_end_to_end_engines(dev, tmp_path):
    """A saved base checkpoint through EffRecognizer, the Recognizer pipeline and the classifier; top-1 ids against a planted-glyph
    index are the same in fp16 and fp32."""
    from effocr_amd.classifiers import AutoClassifierFactory
    from effocr_amd.encoders import AutoEncoderFactory
    from effocr_amd.knn import FaissKNN, IndexFlatIP
    from effocr_amd.pipeline import Recognizer
    from effocr_amd.recognizer_engine import EffRecognizer
    n, ncls = 8, 7
    sd = _sd(ARCH, 224, 7, num_classes=ncls)
    ckpt = tmp_path / "enc_best.pth"
    W.save_checkpoint(sd, ckpt)
    glyphs = _crops(n, 224, 31)
    q = glyphs + 0.05 * torch.randn(glyphs.shape, generator=torch.Generator().manual_seed(32))
    want = torch.arange(n) + 250
    chars = [chr(0x4E00 + i) for i in range(500 + n)]
    dis = F.normalize(torch.randn(500, 768, generator=torch.Generator().manual_seed(9)), dim=1)

    ids = {}
    for prec in ("fp32", "fp16"):
        er = EffRecognizer(str(ckpt), precision=prec, device=dev)
        assert er.arch == ARCH and er.crop_dtype == torch.float32 and er.call_size_invariant
        if prec == "fp32":                                 # the index holds the glyphs' fp32 embeddings among 500 distractors
            planted = torch.from_numpy(er.run(glyphs.numpy())[0])
            cos = F.normalize(planted, dim=1) @ F.normalize(planted, dim=1).T
            assert (cos - 2 * torch.eye(n)).max() < 0.99   # the glyphs are told apart
            index = torch.cat([dis[:250], F.normalize(planted, dim=1), dis[250:]])
        emb = er.run(q.numpy())[0]
        assert emb.shape == (n, 768) and emb.dtype == np.float32
        ids[prec] = (F.normalize(torch.from_numpy(emb), dim=1) @ index.T).argmax(dim=1)
        assert torch.equal(ids[prec], want)
    assert torch.equal(ids["fp16"], ids["fp32"])

    enc = AutoEncoderFactory("timm", ARCH).load(str(ckpt))
    enc.to(dev).eval()
    knn = FaissKNN(index_init_fn=IndexFlatIP, reset_before=False, reset_after=False)
    knn.train(index)
    rec = Recognizer(enc, knn, chars, knn=10)
    _, _, text = rec(q.to(dev))
    assert text == "".join(chars[i] for i in want.tolist())

    clf = AutoClassifierFactory("timm", ARCH, n_classes=ncls).load(str(ckpt))
    clf.to(dev).eval()
    lg = clf(q.to(dev))
    assert lg.shape == (n, ncls)
    want_lg = clf.embed(q.to(dev)) @ sd["head.weight"].to(dev).T + sd["head.bias"].to(dev)
    torch.testing.assert_close(lg, want_lg, rtol=1e-4, atol=1e-4)
    assert torch.equal(clf.predict(q.to(dev)), lg.argmax(dim=1))
    clf.check_status()
