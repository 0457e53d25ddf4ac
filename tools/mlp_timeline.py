#!/usr/bin/env python
"""Per-panel timeline of the fused proj+MLP kernel from a -DMLP_STAMP build (tools/ab_build.sh stamp "-DMLP_STAMP" mlp_bf16p.hip mlp_bf16pair.hip):
   EFFOCR_HIP_LIB=$PWD/tools/ab/lib_stamp.so python tools/mlp_timeline.py [batch]
Prints the mean share of each segment of a whole panel (s_memtime ticks, wave 0) and the per-CU turn-around between workgroups.
--gantt (a -DMLP_STAMP -DMLP_STAMP_ALL=true build: every workgroup of the launch stamps, split parts included): the launch-level schedule of
the last fused-MLP launch instead — end of launch in panel-times, CU-time asleep in the start spread, CU-time in split parts, idle CU-time at
the end.  --tail-first N / --stagger N / --min-rounds N set the mlp_tail_first / mlp_stagger / mlp_stagger_min_rounds options first."""
import ctypes, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from effocr_amd import _lib
from effocr_amd.encoders import HipEncoder
from effocr_amd.weights import init_state_dict

B = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
GANTT = "--gantt" in sys.argv
OPTS = {opt: int(sys.argv[sys.argv.index(flag) + 1]) for flag, opt in (("--tail-first", "mlp_tail_first"), ("--stagger", "mlp_stagger"), ("--min-rounds", "mlp_stagger_min_rounds")) if flag in sys.argv}
PAIR = "--pair" in sys.argv                    # 64-token wave-pair panels (calls of <= 83 crops): every workgroup of the launch stamps
dev = torch.device("cuda:0")
enc = HipEncoder("vit_small_patch16_224", init_state_dict("vit_small_patch16_224", seed=0, img_size=224), img_size=224, precision="bf16", device=dev)
if PAIR:
    enc.set_option("mlp_pair", 1); enc.set_option("cls_only_last", 0)
for k, v in OPTS.items():
    enc.set_option(k, v)
if GANTT:
    enc.split_streams = False                  # one call reaches the launcher whole
    enc.set_option("cls_only_last", 0)         # the last block's launch is a full one too: the table holds ONE launch, every row of it
x = torch.randn(B, 3, 224, 224, device=dev)
for _ in range(3):
    enc.forward(x, normalize=True)
torch.cuda.synchronize()
lib = ctypes.CDLL(os.environ["EFFOCR_HIP_LIB"])
NW, NS = 2048, 20
buf = (ctypes.c_ulonglong * (NW * NS))()
rc = (lib.effocr_debug_mlp_pair_stamps if PAIR else lib.effocr_debug_mlp_stamps)(buf, NW * NS)   # (the pair kernels live in a translation unit of their own: its table)
assert rc == 0, rc
t = np.frombuffer(buf, dtype=np.uint64).reshape(NW, NS).astype(np.int64)
npan = (B * 197 + 127) // 128


def gantt(t):
    """t: the stamp rows of ONE launch by block id.  Times across CUs use the 100 MHz real-time counter (slots 14 / 16: s_memtime is per XCD);
    a workgroup's start wait (s_memtime slots 0 -> 1) is converted with its own ticks-per-real-tick ratio."""
    tail = npan % 256
    split = next((c for c in (6, 4, 2) if 0 < tail and tail * c <= 256), 1)
    grid = npan - tail + tail * split if split > 1 else npan
    t = t[:grid]
    part = (t[:, 19] & 1) == 1
    t0 = t[:, 14].min()
    beg, end = (t[:, 14] - t0).astype(np.float64), (t[:, 16] - t0).astype(np.float64)
    ratio = (end - beg) / np.maximum(t[:, 11] - t[:, 0], 1)
    wait = (t[:, 1] - t[:, 0]) * ratio                                   # start wait, real-time ticks
    run = end - beg - wait
    T = np.median(run[~part])                                             # one panel-time
    hw = t[:, 15]
    cu = ((hw >> 32) & 0xf) * 4096 + ((hw >> 13) & 0x7) * 256 + ((hw >> 8) & 0xf) * 16 + ((hw >> 12) & 1)
    cus = np.unique(cu)
    last = np.array([end[cu == c].max() for c in cus])
    first = np.array([beg[cu == c].min() for c in cus])
    busy = np.array([(end[cu == c] - beg[cu == c]).sum() for c in cus])
    L = end.max()
    print(f"launch of {grid} workgroups ({(~part).sum()} whole panels + {part.sum()} parts, {split}-way) on {len(cus)} CUs; options {OPTS}")
    print(f"  panel-time T = {T:.0f} real-time ticks of 10 ns ({np.median((t[:, 11] - t[:, 1])[~part]):.0f} s_memtime ticks); no-overhead bound {npan / 256:.2f} T")
    print(f"  end of launch                 {L / T:6.3f} T   (first workgroup entry -> last exit)")
    print(f"  CU-time asleep (start spread) {wait.sum() / T:7.2f} T in all = {wait.sum() / T / len(cus):.3f} T per CU  (workgroups that waited: {(wait > 0.01 * T).sum()}, longest {wait.max() / T:.3f} T)")
    if part.any():
        fp = part & (np.arange(grid) < 256)
        print(f"  CU-time in split parts        {run[part].sum() / T:7.2f} T in all = {run[part].sum() / T / len(cus):.3f} T per CU  (a part: mean {run[part].mean() / T:.3f} T, p10 {np.percentile(run[part], 10) / T:.3f}, p90 {np.percentile(run[part], 90) / T:.3f}"
              + (f"; the {fp.sum()} of the first round {run[fp].mean() / T:.3f}, the others {run[part & ~fp].mean() / T:.3f}" if fp.any() and (part & ~fp).any() else "") + ")")
        print(f"  first part enters at {beg[part].min() / T:.3f} T, last whole panel exits at {end[~part].max() / T:.3f} T, parts per CU max {max(int((part & (cu == c)).sum()) for c in cus)}")
    print(f"  idle CU-time at the end       {(L - last).sum() / T:7.2f} T in all = {(L - last).mean() / T:.3f} T per CU  (p10 {np.percentile(L - last, 10) / T:.3f}, p90 {np.percentile(L - last, 90) / T:.3f}, max {(L - last).max() / T:.3f})")
    print(f"  idle CU-time at the start     {first.sum() / T:7.2f} T in all; between workgroups {(last - first - busy).sum() / T:.2f} T in all")
    print(f"  whole panels per CU: min {min(int((~part & (cu == c)).sum()) for c in cus)}, max {max(int((~part & (cu == c)).sum()) for c in cus)}; whole-panel run time p10 {np.percentile(run[~part], 10) / T:.3f} T, p90 {np.percentile(run[~part], 90) / T:.3f} T")
    # the ragged end: when the CUs finish their last whole panel
    lw = np.array([end[~part & (cu == c)].max() for c in cus if (~part & (cu == c)).any()])
    print(f"  CUs finish their last whole panel between {lw.min() / T:.3f} T and {lw.max() / T:.3f} T (mean {lw.mean() / T:.3f} T)")


if GANTT:
    gantt(t)
    sys.exit(0)
main = npan - npan % 256 if (npan % 256) * 2 <= 256 else npan
t = t[:(B * 197 + 63) // 64] if PAIR else t[8:main]   # (the CLS-only launch of the last block rewrote the first 8 rows)
names = ["stagger wait", "requests issued + params to regs", "params -> LDS + barrier", "rows/attn/stage 0 landed", "projection MFMAs", "bias + LayerNorm",
         "A(0) + park", "rolled loop", "last A/B + gelu + B", "x stores issued", "second output", "stores acked"]
tot = t[:, 11] - t[:, 1]
print(f"{len(t)} whole panels; ticks per panel (after the start spread) mean {tot.mean():.0f} (min {tot.min()}, max {tot.max()}); start spread mean {(t[:, 1] - t[:, 0]).mean():.0f}")
for i in range(2, 12):
    seg = t[:, i] - t[:, i - 1]
    print(f"  {names[i]:42s} {seg.mean():9.0f}  {100 * seg.mean() / tot.mean():5.1f} %   (p10 {np.percentile(seg, 10):.0f}, p90 {np.percentile(seg, 90):.0f})")
print(f"  projection by output group (stamps 17, 18): group 0 {(t[:, 17] - t[:, 3]).mean():.0f}, group 1 {(t[:, 18] - t[:, 17]).mean():.0f}, group 2 {(t[:, 4] - t[:, 18]).mean():.0f} ticks (96 MFMAs = 3 072 each)")
print(f"  mid-stage waits of one wave, sum over the panel's {12 * 12 + 18} stages: vmcnt {t[:, 12].mean():.0f} ticks, barrier {t[:, 13].mean():.0f} ticks")
xcc = (t[:, 15] >> 32) & 0xf                     # s_memtime is per XCD: concurrency inside each XCD (32 CUs), then averaged
cm, mx, fr = [], [], []
for xc in np.unique(xcc):
    tt = t[xcc == xc]
    ev = np.concatenate([np.stack([tt[:, 1], np.ones(len(tt))], 1), np.stack([tt[:, 2], -np.ones(len(tt))], 1)])
    ev = ev[np.argsort(ev[:, 0])]
    conc = np.cumsum(ev[:, 1]); dt = np.diff(ev[:, 0])
    cm.append((conc[:-1] * dt).sum() / dt.sum()); mx.append(conc.max()); fr.append(len(tt))
print(f"  workgroups in the prologue wait at once, per XCD of 32 CUs (time-weighted over the launch): mean {np.mean(cm):.1f}, max {np.max(mx):.0f}  (XCDs seen {len(cm)}, panels per XCD {np.mean(fr):.0f})")
# per-CU turn-around: group by (xcc, se, cu) and sort by start
hw = t[:, 15]
cu = ((hw >> 32) & 0xf) * 4096 + ((hw >> 13) & 0x7) * 256 + ((hw >> 8) & 0xf) * 16 + ((hw >> 12) & 1)
gaps = []
for c in np.unique(cu):
    rows = t[cu == c]
    rows = rows[np.argsort(rows[:, 0])]
    gaps += list(rows[1:, 0] - rows[:-1, 11])
gaps = np.array(gaps)
print(f"CUs seen {len(np.unique(cu))}; turn-around end(stores acked) -> next workgroup's entry on the same CU: mean {gaps.mean():.0f}, p10 {np.percentile(gaps, 10):.0f}, p90 {np.percentile(gaps, 90):.0f} ticks")
