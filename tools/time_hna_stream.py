"""Cost of streaming the harmonic-plus-noise analysis (analysis_stream.HarmonicNoiseStream) at the recipe -- B = 32, two
seconds in blocks of 2400 samples, hop 240, K = 155, n_mag = 256, f0 one block late -- next to the one-shot call on the same
(x, f0), dev tool; bench.py is the contract.  Writes profiles/hna_stream_timing.txt, or the file given as the first argument.

Default: HIP events around whole utterances (20 pushes, the late f0, finish) and around back-to-back one-shot calls, 3 warm-up
rounds, the median of 5 windows with the two alternating inside each round; the results of the two are compared with
torch.equal first.  These are call times: a push is host work (concatenation, slicing, allocation) around a kernel of a few
microseconds.

The kernel time is taken in runs of their own under ``rocprofv3 --kernel-trace --stats``: ``--only stream`` streams REPS
utterances and nothing else, ``--only one-shot`` makes REPS one-shot calls and nothing else; harm_analysis_kernel's total in the
statistics over REPS is the kernel time per utterance.  ``--kernel-us STREAM ONE_SHOT`` appends the two figures to the file."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

B, SR, HOP, K, N_MAG, T, BLOCK, REPS = 32, 24000.0, 240, 155, 256, 48000, 2400, 20
OUT = os.path.join(ROOT, "profiles", "hna_stream_timing.txt")
argv = sys.argv[1:]
if argv and not argv[0].startswith("--"):
    OUT = argv.pop(0)
if argv[:1] == ["--kernel-us"]:
    with open(OUT, "a") as f:
        f.write(f"kernel time per utterance (rocprofv3 --kernel-trace --stats, total of harm_analysis_kernel over {REPS} utterances "
                f"/ {REPS}, one run each): stream (21 launches) {float(argv[1]):.1f} us, one-shot (1 launch) {float(argv[2]):.1f} us\n")
    sys.exit(0)

from golf_amd import functional as GF
from golf_amd.analysis_stream import HarmonicNoiseStream
from golf_amd.hna import HarmonicNoiseAnalysis


def inputs(device, seed=0):
    """Harmonic rows with noise and their f0 tracks in Hz: slow glides between 80 and 400 Hz, a third of the frames unvoiced
    (the signals of tools/time_hna.py)."""
    g = torch.Generator().manual_seed(seed)
    F = T // HOP + 1
    lo = 95.0 * (345.0 / 95.0) ** torch.rand(B, 1, generator=g)
    f0 = lo * (1 + 0.15 * torch.sin(torch.arange(F) * 0.05 + 6.28 * torch.rand(B, 1, generator=g)))
    up = torch.nn.functional.interpolate(f0[:, None], size=(F - 1) * HOP + 1, mode="linear", align_corners=True)[:, 0]
    ph = torch.cumsum(up.double() / SR, 1)[:, :T]
    x = sum(torch.sin(2 * math.pi * h * ph) / h for h in range(1, 25)).float() * 0.3 + 0.05 * torch.randn(B, T, generator=g)
    unvoiced = (torch.arange(F)[None] // 10 + torch.arange(B)[:, None]) % 3 == 0
    return x.to(device), torch.where(unvoiced, torch.zeros(()), f0).float().to(device)


x, f0 = inputs("cuda")
F, PER = f0.shape[1], BLOCK // HOP
module = HarmonicNoiseAnalysis(SR, HOP, K, n_mag=N_MAG).cuda()
st = HarmonicNoiseStream(module, B)
blocks = [x[:, i:i + BLOCK] for i in range(0, T, BLOCK)]
late = [f0[:, max(i - 1, 0) * PER:i * PER] for i in range(len(blocks))]   # the frames of the block before


def one_shot():
    return GF.harmonic_analysis(x, f0, SR, HOP, K, n_mag=N_MAG)


def stream():
    outs = [st.push(b, f) for b, f in zip(blocks, late)]
    outs.append(st.push(f0=f0[:, (len(blocks) - 1) * PER:]))
    outs.append(st.finish())
    return outs


if argv[:1] == ["--only"]:
    fn = {"stream": stream, "one-shot": one_shot}[argv[1]]
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    sys.exit(0)

ref, outs = one_shot(), stream()
frames = [o[0].shape[1] for o in outs]
for i in range(2):
    assert torch.equal(torch.cat([o[i].as_tensor() for o in outs], 1), ref[i])


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for fn in (one_shot, stream):
    timed(fn, 3)
samples = {"one-shot": [], "stream": []}
for rep in range(5):
    samples["one-shot"].append(timed(one_shot, REPS))
    samples["stream"].append(timed(stream, REPS))
med = {k: statistics.median(s) for k, s in samples.items()}
with open(OUT, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: HarmonicNoiseStream B={B} T={T} hop={HOP} K={K} n_mag={N_MAG} ({B * F} frames), "
            f"{len(blocks)} pushes of {BLOCK} samples with the f0 of the block before, the last f0 frames, finish(); frames per "
            f"call {frames}; equal to the one-shot call bit for bit; HIP events around whole utterances, 3 warm-up rounds, median "
            f"of 5 windows ({REPS} utterances and {REPS} one-shot calls each, alternating), us\n")
    f.write(f"one-shot harmonic_analysis, per call      {med['one-shot']:10.1f}   (min {min(samples['one-shot']):.1f}, max {max(samples['one-shot']):.1f})\n")
    f.write(f"stream, per utterance ({len(outs)} calls)          {med['stream']:10.1f}   (min {min(samples['stream']):.1f}, max {max(samples['stream']):.1f})\n")
    f.write(f"stream, per call                          {med['stream'] / len(outs):10.1f}\n")
print(open(OUT).read())
