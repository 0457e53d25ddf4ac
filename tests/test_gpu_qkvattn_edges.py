"""-m gpu: the fused qkv + attention kernel (csrc/qkvattn.hip) at every body its projection schedule has — the first and last ring stage
of a q / k / v section run row-block-major and host the hand-over (accumulators + bias -> 16-bit operand fragments -> registers / LDS)
of the finished row block in the gaps of the other block's MFMAs (QA_EDGE_BLOCK_MAJOR).  Through HipEncoder's public interface only:
  * two-tile and one-tile wave bodies, 7 token tiles (ViT-S/16 at 224: 197 tokens), all-token and class-token variant   -> oracle parity
  * one head per workgroup (B = 1), head split (B = 5, B = 260), persistent workgroups that run two images (B = 576: the
    path that requests the next image's rows, and the path whose weight ring runs dry)                                    -> same bits
  * short images (17 / 50 tokens: the 2-tile instantiation, dummy tiles, compare-and-select key masking)                  -> oracle parity
  * the 128-wide miniature (a section is ONE ring stage: it keeps the k-step-major order)                                 -> oracle parity
A hand-over that raced with the previous head's attention reads of K / V in LDS, or a hosted slice that read an accumulator before its
last MFMA, would show as a mismatch between the work splits or against the oracle.
"""
import pytest
import torch

from effocr_amd.weights import init_state_dict
from oracle.encoders_ref import encoder_forward

pytestmark = pytest.mark.gpu

# max-norm relative error of the default dispatch against oracle A (plain torch fp32 on the CPU): the bounds of tests/test_gpu_encoder.py
REL = {"fp16": 1e-3, "bf16": 8e-3}
VIT_S = "vit_small_patch16_224"


def rel_err(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


def against_oracle(arch, img, B, prec, dev, seed):
    from effocr_amd.encoders import HipEncoder
    sd = init_state_dict(arch, seed=seed, img_size=img)
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(seed + 100))
    ref = encoder_forward(arch, sd, x)
    got = HipEncoder(arch, sd, img_size=img, precision=prec, device=dev).forward(x.to(dev)).cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    e = rel_err(got, ref)
    print(f"{arch} img {img} {prec} B={B}: rel err {e:.3e} (bound {REL[prec]:.0e})")
    return e


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_oracle_parity_default_dispatch(dev, prec):
    assert against_oracle(VIT_S, 224, 3, prec, dev, seed=2) <= REL[prec]


def crops(dev, n):
    return torch.randn(n, 3, 224, 224, generator=torch.Generator(device=dev).manual_seed(31), device=dev)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_determinism_and_one_head_per_workgroup(dev, prec):
    """Two consecutive 5-crop forwards give the same bits, and so do the 5 crops as calls of their own (B = 1: head split 6, one head per
    workgroup, every head-rotation start offset)."""
    from effocr_amd.encoders import HipEncoder
    enc = HipEncoder(VIT_S, init_state_dict(VIT_S, seed=3, img_size=224), precision=prec, device=dev)
    x = crops(dev, 5)
    five = enc.forward(x)
    assert torch.isfinite(five).all()
    assert torch.equal(five, enc.forward(x)), "two consecutive forwards of the same 5 crops differ"
    one = torch.cat([enc.forward(x[i:i + 1].contiguous()) for i in range(5)])
    assert torch.equal(one, five)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_every_work_split_gives_the_same_bits(dev, prec):
    """The same 5 crops as calls of their own, as a 5-crop call and as the first rows of a 260-crop call: identical embeddings, bit for bit.

    The fused qkv + attention kernel is bit-identical for any work split; the fused MLP beside it is not at its defaults — below a round
    of CUs it sums the hidden dimension in split parts, in another fp32 order (tests/test_gpu_encoder.py::
    test_embedding_does_not_depend_on_the_call_size bounds that: 1.1e-2 bf16 / 1.4e-3 fp16 between a 5- and a 260-crop call) — so the
    encoder's `tail_split` switch keeps the MLP on whole 128-token panels, the form the 1024-crop headline runs, at every call size.  What
    still changes with the call size is this kernel's work split alone:
      B = 1    head split 6, one head per workgroup, every head-rotation start offset
      B = 5    head split 6, 30 workgroups
      B = 260  as ONE call (no stream split): 256 one-image workgroups + a head-split second launch of the last 4 images;
               with the head split off: 256 persistent workgroups, the first 4 run two images (rows 0..3 are their FIRST images: the
               path that requests the next image's rows; row 4 runs the path whose weight ring runs dry);
               as the default dispatch cuts it: two concurrent 130-crop calls on side streams."""
    from effocr_amd.encoders import HipEncoder
    enc = HipEncoder(VIT_S, init_state_dict(VIT_S, seed=3, img_size=224), precision=prec, device=dev)
    enc.set_option("tail_split", 0)
    x = crops(dev, 260)
    five = enc.forward(x[:5].contiguous())
    got = {"B = 1": torch.cat([enc.forward(x[i:i + 1].contiguous()) for i in range(5)]),
           "B = 260, two streams": enc.forward(x)[:5]}
    enc.split_streams = False
    got["B = 260, one call"] = enc.forward(x)[:5]
    enc.set_option("qa_hsplit", 1)
    got["B = 260, two-image workgroups"] = enc.forward(x)[:5]
    assert torch.isfinite(five).all()
    for name, e in got.items():
        print(f"{prec} {name} against B = 5: max |diff| {(e - five).abs().max().item():.3e}, equal {torch.equal(e, five)}")
    for name, e in got.items():
        assert torch.equal(e, five), name


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_first_and_second_image_of_a_persistent_workgroup(dev, prec):
    """576 crops in ONE call of the library (no stream split): 512 run as two images on each of 256 persistent workgroups — the first
    image's last head requests the next image's rows, the second image's last head lets the weight ring run dry — and 64 as a head-split
    tail launch.  The same 5 crops as first images (rows 0..4) and as second images (rows 256..260) of their workgroups: identical bits."""
    from effocr_amd.encoders import HipEncoder
    enc = HipEncoder(VIT_S, init_state_dict(VIT_S, seed=3, img_size=224), precision=prec, device=dev)
    x = crops(dev, 576)
    x[256:261] = x[:5]
    e = enc.forward(x)
    assert torch.isfinite(e).all()
    assert torch.equal(e[256:261], e[:5])
    assert torch.equal(e, enc.forward(x))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("img", [64, 112])
def test_short_images(dev, img, prec):
    assert against_oracle(VIT_S, img, 2, prec, dev, seed=4) <= REL[prec]


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("B", [2, 70])
def test_miniature_width(dev, B, prec):
    assert against_oracle("vit_tiny_test", 64, B, prec, dev, seed=5) <= REL[prec]
