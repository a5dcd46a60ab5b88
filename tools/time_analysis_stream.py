"""Host-side times of the streaming analysis (golf_amd/analysis_stream.py, csrc/f0_viterbi_stream.hip) at B = 32 and the
recipe's analysis (24 kHz, hop 240, 60 - 1000 Hz, K = 7; LPC order 22, W = 960), dev tool; bench.py is the contract.  Writes
profiles/analysis_stream_timing.txt, or the file given as the first argument.

A host clock around a loop of calls that ends in a device synchronise, 50 warm-up calls, the median of five windows with the
variants alternating inside each round: one push of one hop in steady state for each stream (the lag-1024 tracker after 1 200
frames, so that every push walks 1 024 backpointers), a 2 s utterance pushed in one block beside the one-shot F0Tracker, and
the two path calls alone on that utterance's candidates.  The lag-1024 stream is checked bitwise against the one-shot."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from golf_amd import functional as GF
from golf_amd.analysis_stream import F0Stream, F0TrackerStream, LPCAnalysisStream
from golf_amd.f0 import F0Analysis, F0Tracker
from golf_amd.lpc import LPCAnalysis

B, SR, HOP = 32, 24000, 240
torch.manual_seed(0)
t = torch.arange(2 * SR, device="cuda") / SR
f0s = torch.linspace(90, 380, B, device="cuda")[:, None]
x = sum(torch.sin(2 * torch.pi * f0s * h * t) / h for h in range(1, 8)) + 0.05 * torch.randn(B, 2 * SR, device="cuda")
yin, trk, lpc = F0Analysis(SR, HOP).cuda(), F0Tracker(SR, HOP).cuda(), LPCAnalysis(22, HOP).cuda()
res = {}


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def report(name, samples):
    res[name] = dict(median_us=round(statistics.median(samples), 1), min_us=round(min(samples), 1), max_us=round(max(samples), 1))
    print(name, res[name], flush=True)


# ---- one push of one hop, steady state -----------------------------------------------------------------------------------
streams = {"F0Stream": F0Stream(yin, B), "F0TrackerStream lag 8": F0TrackerStream(trk, B),
           "F0TrackerStream lag 1024": F0TrackerStream(trk, B, lag=1024), "LPCAnalysisStream": LPCAnalysisStream(lpc, B)}
x_long = x.repeat(1, 60)         # 120 s: no stream comes to the end of its input inside a timed window
prime = {name: 4800 for name in streams}   # past the first frames: every later hop completes one frame
prime["F0TrackerStream lag 1024"] = 12 * SR   # 1200 frames consumed: every later hop decides a frame 1024 frames back
pos = {}
for name, s in streams.items():
    s.push(x_long[:, :prime[name]])
    pos[name] = prime[name]


def push_hop(name):
    out = streams[name].push(x_long[:, pos[name]:pos[name] + HOP])
    pos[name] += HOP
    assert pos[name] <= x_long.shape[1] and out[0].shape[1] == 1 if isinstance(out, tuple) else out.shape[1] == 1
    return out


for name in streams:
    timed(lambda: push_hop(name), 50)   # warm-up
samples = {name: [] for name in streams}
for rep in range(5):
    for name in streams:
        samples[name].append(timed(lambda: push_hop(name), 1500))
for name in streams:
    report("push of one hop: " + name, samples[name])
for s in streams.values():
    s.finish()

# ---- a 2 s utterance in one block ------------------------------------------------------------------------------------------
s8, s1024 = F0TrackerStream(trk, B), F0TrackerStream(trk, B, lag=1024)


def whole(s):
    a = s.push_all(x)
    b = s.finish_all()
    return a, b


runs = {"one-shot F0Tracker": lambda: trk.analyse(x), "F0TrackerStream lag 8, one block + finish": lambda: whole(s8),
        "F0TrackerStream lag 1024, one block + finish": lambda: whole(s1024)}
one = trk.analyse(x)
a, b = whole(s1024)
assert torch.equal(torch.cat([a[0], b[0]], 1), one[0]) and torch.equal(torch.cat([a[1], b[1]], 1), one[1])
a, b = whole(s8)
print("frames", one[0].shape[1], "states that differ at lag 8:", int((torch.cat([a[1], b[1]], 1) != one[1]).sum()))
for fn in runs.values():
    timed(fn, 20)
samples = {name: [] for name in runs}
for rep in range(5):
    for name, fn in runs.items():
        samples[name].append(timed(fn, 100))
for name in runs:
    report("2 s utterance: " + name, samples[name])

# ---- the path kernels alone on the utterance's candidates -----------------------------------------------------------------------
cp, ca = one[2], one[3]
F = cp.shape[1]
carries = {lag: GF.f0_viterbi_stream_state(B, 7, lag, "cuda") for lag in (8, 1024)}
paths = {"f0_viterbi (one-shot path kernel)": lambda: GF.f0_viterbi(cp, ca, SR, 24.0, return_state=True),
         "f0_viterbi_stream lag 8, one call with flush": lambda: GF.f0_viterbi_stream(cp, ca, carries[8], 0, 8, SR, 24.0, flush=True, return_state=True),
         "f0_viterbi_stream lag 1024, one call with flush": lambda: GF.f0_viterbi_stream(cp, ca, carries[1024], 0, 1024, SR, 24.0, flush=True, return_state=True)}
for fn in paths.values():
    timed(fn, 50)
samples = {name: [] for name in paths}
for rep in range(5):
    for name, fn in paths.items():
        samples[name].append(timed(fn, 1000))
for name in paths:
    report(f"path alone, {F} frames: " + name, samples[name])
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "analysis_stream_timing.txt")
with open(out, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}; B = {B}, {SR} Hz, hop {HOP}; microseconds per call: median (min - max) of 5 windows\n")
    for name, r in res.items():
        f.write(f"{name}: {r['median_us']} ({r['min_us']} - {r['max_us']})\n")
