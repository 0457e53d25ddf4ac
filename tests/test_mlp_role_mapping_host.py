"""The fused MLP's launch-level role mapping (effocr_amd/csrc/mlp_roles.hpp) on the host: the header is plain C++, so a small stand-alone
program (host compiler, AddressSanitizer + UBSan where the compiler has them) prints the role of every block id of a launch and the
checks below run over that table.  For every (panel count, split, tail_first):
  * every whole panel and every (tail panel, part) is produced exactly once, and no panel of the full rounds becomes a part;
  * tail_first = 0 is the old rule  bid < main_wgs ? whole(bid) : part(bid - main_wgs);
  * out-of-range tail_first values clamp (to every part / the first round, down to a multiple of 8; negative = 0);
  * with tail_first > 0 the parts that run first sit on the last tail_first ids of the first round, in order."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR_DIR = os.path.join(ROOT, "effocr_amd", "csrc")
SLOTS = 256

MAIN = r"""
#include "mlp_roles.hpp"
#include <cstdio>
#include <cstdlib>
// argv: main_panels tail split slots tail_first  ->  line 1: the clamped tail_first; then "part index" per block id
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const int main_panels = std::atoi(argv[1]), tail = std::atoi(argv[2]), split = std::atoi(argv[3]), slots = std::atoi(argv[4]), tf = std::atoi(argv[5]);
  std::printf("%d\n", effocr::mlp_tail_first_clamp(tf, main_panels, tail, split, slots));
  const int grid = main_panels + tail * split;
  for (int bid = 0; bid < grid; ++bid) {
    const effocr::MlpRole r = effocr::mlp_role(bid, main_panels, tail, split, slots, tf);
    std::printf("%d %d\n", r.part ? 1 : 0, r.index);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def role_prog(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("mlp_roles")
    src, exe = d / "roles_main.cpp", d / "roles_main"
    src.write_text(MAIN)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", HDR_DIR, str(src), "-o", str(exe)]
    res = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if res.returncode != 0 or subprocess.run([str(exe), "256", "1", "2", "256", "0"], capture_output=True).returncode != 0:
        res = subprocess.run(base, capture_output=True, text=True)      # a compiler without the sanitizer runtimes: plain build
    assert res.returncode == 0, res.stderr
    return str(exe)


def _launch(npanels, split):
    """(main_panels, tail) as launch_mlp cuts a call of npanels 128-token panels whose tail is split `split`-ways."""
    tail = npanels % SLOTS
    assert 0 < tail and tail * split <= SLOTS
    return npanels - tail, tail


def _roles(prog, main_panels, tail, split, tf, slots=SLOTS):
    out = subprocess.run([prog, str(main_panels), str(tail), str(split), str(slots), str(tf)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    return int(lines[0]), [tuple(int(v) for v in ln.split()) for ln in lines[1:] if ln]


def _expected_clamp(tf, tail, split):
    return max(0, min(tf, tail * split, SLOTS)) & ~7


@pytest.mark.parametrize("npanels", [262, 524, 1576, 1537])
@pytest.mark.parametrize("split", [2, 4, 6])
def test_every_piece_exactly_once(role_prog, npanels, split):
    main_panels, tail = _launch(npanels, split)
    parts = tail * split
    old = [(0, b) if b < main_panels else (1, b - main_panels) for b in range(main_panels + parts)]
    for tf in (0, 8, 64, parts, parts + 8, SLOTS + 64, 10 ** 6, 13, -8):
        clamp, roles = _roles(role_prog, main_panels, tail, split, tf)
        assert clamp == _expected_clamp(tf, tail, split), (tf, clamp)
        assert len(roles) == main_panels + parts
        assert sorted(i for p, i in roles if p == 0) == list(range(main_panels)), f"whole panels, tail_first={tf}"
        assert sorted(i for p, i in roles if p == 1) == list(range(parts)), f"(panel, part) pairs, tail_first={tf}"
        if clamp == 0:
            assert roles == old, f"tail_first={tf} must be the old mapping"
            continue
        # first round: the early ids keep their whole panels, the last `clamp` ids run parts 0 .. clamp-1 in order
        assert roles[:SLOTS - clamp] == [(0, b) for b in range(SLOTS - clamp)]
        assert roles[SLOTS - clamp:SLOTS] == [(1, i) for i in range(clamp)]
        # behind it: the remaining whole panels in order, then the remaining parts in order
        assert roles[SLOTS:] == [(0, i) for i in range(SLOTS - clamp, main_panels)] + [(1, i) for i in range(clamp, parts)]


def test_inert_without_first_round_or_split(role_prog):
    # no split tail, no start spread (slots = 0 is how the launcher says so), less than one round of whole panels, odd CU counts
    for main_panels, tail, split, slots in ((512, 12, 1, 256), (512, 0, 6, 256), (512, 12, 6, 0), (200, 12, 6, 256), (512, 12, 6, 252), (1216, 12, 6, 304)):
        clamp, roles = _roles(role_prog, main_panels, tail, split, 64, slots)
        assert clamp == 0
        parts = tail * split if split > 1 else 0
        assert roles[:main_panels + parts] == [(0, b) if b < main_panels else (1, b - main_panels) for b in range(main_panels + parts)]
