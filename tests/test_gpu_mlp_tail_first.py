"""-m gpu: the fused MLP's "mlp_tail_first" option (effocr_amd/csrc/mlp_roles.hpp) changes WHEN the split parts of a launch's tail run —
the first ones in the last start phases of the first round of workgroups instead of at the end — and nothing else: the same parts write
the same partial sums and the reduction adds them in the same fixed order, so embeddings must be bit-identical to mlp_tail_first = 0.

vit_small_patch16_224, bf16 and fp16, one call per launch (no Python-side sub-batches):
  * 170 crops with mlp_stagger_min_rounds = 1: 262 panels = one round of 256 + 6 tail panels cut 6-ways (36 parts; "all" clamps to 32);
  * 340 crops: 524 panels = two rounds + 12 tail panels (72 parts).
Three calls per setting (the order in which workgroups arrive varies from call to call), a clean status word behind each, and one
comparison of the default setting against the library's fp32 mode within the default dispatch's bound of tests/test_gpu_encoder.py."""
import pytest
import torch

from effocr_amd.weights import init_state_dict

pytestmark = pytest.mark.gpu

ARCH, IMG = "vit_small_patch16_224", 224
REL = {"fp16": 1e-3, "bf16": 8e-3}                       # tests/test_gpu_encoder.py REL: the default dispatch against fp32
SHAPES = {170: 1, 340: 2}                                # crops -> mlp_stagger_min_rounds
ALL_PARTS = 1 << 20                                      # clamps to every part of the tail (a multiple of 8)


@pytest.fixture(scope="module")
def state():
    return init_state_dict(ARCH, seed=5, img_size=IMG)


@pytest.fixture(scope="module")
def crops(dev):
    return torch.randn(340, 3, IMG, IMG, generator=torch.Generator().manual_seed(11)).to(dev)


@pytest.fixture(scope="module")
def engines(dev, state):
    from effocr_amd.encoders import HipEncoder
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = HipEncoder(ARCH, state, img_size=IMG, precision=prec, device=dev)
            made[prec].split_streams = False             # one call reaches the launcher whole
        return made[prec]
    return get


def _embed(enc, x, min_rounds, tail_first):
    enc.set_option("mlp_stagger_min_rounds", min_rounds)
    if tail_first is not None:
        enc.set_option("mlp_tail_first", tail_first)
    out = enc.forward(x, normalize=True).clone()
    enc.check_status()
    return out


@pytest.fixture(scope="module")
def baseline(engines, crops):
    """Embeddings with mlp_tail_first = 0, computed once per (precision, call size) and left unchanged."""
    made = {}

    def get(prec, B):
        if (prec, B) not in made:
            made[prec, B] = _embed(engines(prec), crops[:B], SHAPES[B], 0)
        return made[prec, B]
    return get


@pytest.mark.parametrize("tail_first", [8, 32, ALL_PARTS])
@pytest.mark.parametrize("B", sorted(SHAPES))
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_bit_identical_to_tail_last(engines, crops, baseline, prec, B, tail_first):
    ref = baseline(prec, B)
    assert torch.isfinite(ref).all()
    enc = engines(prec)
    try:
        for rep in range(3):
            got = _embed(enc, crops[:B], SHAPES[B], tail_first)
            assert torch.equal(got, ref), f"{prec} B={B} mlp_tail_first={tail_first} call {rep}: {(got != ref).sum().item()} values differ, max |diff| {(got - ref).abs().max().item():.3e}"
    finally:
        enc.set_option("mlp_tail_first", 0)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_default_setting_against_fp32_mode(dev, state, crops, prec):
    from effocr_amd.encoders import HipEncoder
    B = 170
    e32 = HipEncoder(ARCH, state, img_size=IMG, precision="fp32", device=dev)
    ref = e32.forward(crops[:B], normalize=True).clone()
    e32.check_status()
    enc = HipEncoder(ARCH, state, img_size=IMG, precision=prec, device=dev)   # a fresh engine: every option at its default but the two below
    enc.split_streams = False
    got = _embed(enc, crops[:B], SHAPES[B], None)
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"{ARCH} {prec} B={B}, default mlp_tail_first, against the fp32 mode: rel err {err:.3e} (bound {REL[prec]:.0e})")
    assert err <= REL[prec]
