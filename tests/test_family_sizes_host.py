"""Every encoder-family library reports the blob size, the workspace size and the default sub-batch it reported before the families' host
code moved onto the shared cores (csrc/enc_core.hpp: enc_default_chunk; token_core.hpp; resnet_core.hpp): tests/golden/family_sizes.json
was recorded from a build of the commit before that move by tests/golden/make_family_sizes.py, whose record() runs again here.  It covers
every architecture each create accepts, each precision, the smallest image size, 64 and 224, and workspace_bytes(b) on either side of
every default sub-batch cap (b up to 4096), with the default sub-batch and after set_chunk(3).  No GPU is needed."""
import importlib.util
import json
import os

import pytest

from effocr_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def sizes():
    spec = importlib.util.spec_from_file_location("make_family_sizes", os.path.join(GOLDEN, "make_family_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(GOLDEN, "family_sizes.json")) as f:
        return mod, json.load(f), mod.record(os.path.dirname(os.path.abspath(_lib.__file__)))


def test_fixture_covers_every_family_and_architecture(sizes):
    mod, golden, _ = sizes
    want = {f"{fam}/{arch}/{img}/{prec}" for fam, (archs, imgs) in mod.FAMILIES.items() for arch in archs for img in imgs
            for prec in mod.PRECISIONS}
    assert set(golden) == want
    assert sorted(mod.FAMILIES) == ["beit", "bit", "effnet", "mnv3", "resnet", "swin", "vit8"]
    assert all(len(row) == 5 and len(row[3]) == len(row[4]) == len(mod.BATCHES) for row in golden.values())


@pytest.mark.parametrize("fam", ["beit", "bit", "effnet", "mnv3", "resnet", "swin", "vit8"])
def test_sizes_equal_the_recorded_ones(sizes, fam):
    _, golden, now = sizes
    keys = [k for k in golden if k.startswith(fam + "/")]
    assert keys
    for k in keys:
        assert now[k] == golden[k], k
