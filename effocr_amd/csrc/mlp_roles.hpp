// Launch-level schedule of the fused MLP (mlp_kernel.hpp): which piece of work a workgroup of the one launch runs.  Plain C++ — the
// launcher, the kernel entry and the host test (tests/test_mlp_role_mapping_host.py) share these functions.
//
// A launch is `main_panels` whole 128-token panels + `tail` panels of the last, partially filled round cut `split`-ways along the hidden
// dimension (tail * split parts), one workgroup each, one workgroup per CU (`slots` CUs).  Block ids are dispatched in order and dealt
// round-robin over the 8 XCDs, so the first `slots` ids are the first round and (bid >> 3) & 31 is an id's start phase there.
//
//   tail_first == 0:  ids [0, main_panels) run the whole panels, the ids behind them the parts (dispatched last).
//   tail_first  > 0:  the LAST tail_first ids of the first round — its last tail_first / 8 start phases — run parts [0, tail_first)
//                     instead of sleeping through their share of the start spread: a CU that first runs a part is offset by a part's time
//                     for the rest of the launch.  Every id behind the first round runs the remaining whole panels in order, then the
//                     remaining parts.  Only the order changes: every panel and every (panel, part) still runs exactly once, a panel of
//                     the full rounds never becomes a part, and the parts' partial sums are reduced in the same fixed order.
#pragma once

namespace effocr {

struct MlpRole {
  bool part;                                             // false: whole panel `index`; true: split part `index` = (tail panel index / split, part index % split)
  int index;
};

// tail_first as the launch can honour it: a multiple of 8 (whole start phases), at most every part and at most the first round; 0 where
// there is no split tail, no first round of `slots` whole panels to take the ids from, or the phases are not the 32 x 8 the spread assumes
constexpr int mlp_tail_first_clamp(int tail_first, int main_panels, int tail, int split, int slots) {
  if (tail_first <= 0 || tail <= 0 || split <= 1 || slots <= 0 || slots > 256 || slots % 8 != 0 || main_panels < slots) return 0;
  int tf = tail_first < tail * split ? tail_first : tail * split;
  if (tf > slots) tf = slots;
  return tf & ~7;
}

// the mapping for a tail_first that mlp_tail_first_clamp has passed (what the launcher hands the kernel: three scalar compares at the
// kernel's entry).  Needs slots <= main_panels; slots = 0 where the launch has no start spread.  tf = 0 is the order without the
// option:  bid < main_panels ? whole(bid) : part(bid - main_panels)
constexpr MlpRole mlp_role_clamped(int bid, int main_panels, int slots, int tf) {
  // (selects, not early returns: in the kernel the two bodies hang on ONE scalar branch, as they did on  bid < main_wgs)
  const int lo = slots - tf;
  const bool early = bid < lo;                                       // first round, early phases: whole panel bid (behind its start wait)
  const bool first = bid < slots;                                    // first round, last phases: part bid - lo first
  const bool rest = bid < main_panels + tf;                          // then the remaining whole panels (bid - tf), then the remaining parts
  const int index = early ? bid : first ? bid - lo : rest ? bid - tf : bid - main_panels;
  return MlpRole{!(early | (rest & !first)), index};
}

constexpr MlpRole mlp_role(int bid, int main_panels, int tail, int split, int slots, int tail_first) {
  const int tf = mlp_tail_first_clamp(tail_first, main_panels, tail, split, slots);
  return mlp_role_clamped(bid, main_panels, tf > 0 ? slots : 0, tf);
}

}  // namespace effocr
