"""Cost of the fused residual and of streaming the spectral-envelope, residual and glottal-source analyses
(functional.ltv_residual; analysis_stream.SpectralEnvelopeStream / ResidualStream / GlottalSourceStream) at the recipe --
B = 32, two seconds, hop 240, M = 22, blocks of 2400 samples with the frame-rate inputs one block late -- next to the one-shot
calls on the same inputs, dev tool; bench.py is the contract.  Writes profiles/env_glottal_stream_timing.txt, or the file given
as the first argument.

Default: HIP events around whole utterances (20 pushes, the late frames, finish) and around back-to-back one-shot calls, 3
warm-up rounds, the median of 5 windows with the versions alternating inside each round; every stream's result is compared
with its one-shot with torch.equal first.  These are call times: a push is host work (concatenation, slicing, allocation)
around kernels of a few microseconds.  The fused residual is timed against the chain it replaces, ``ltv_inverse`` +
``linear_upsample`` + a divide, in the same windows.

Kernel times are taken in runs of their own under ``rocprofv3 --kernel-trace --stats``: ``--only NAME`` runs REPS rounds of one
version and nothing else; ``--kernel-stats NAME CSV`` appends the total of every kernel in that run's statistics over REPS."""
import csv
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, SR, HOP, M, T, BLOCK, REPS = 32, 24000.0, 240, 22, 48000, 2400, 20
OUT = os.path.join(ROOT, "profiles", "env_glottal_stream_timing.txt")
argv = sys.argv[1:]
if argv and not argv[0].startswith("--"):
    OUT = argv.pop(0)
if argv[:1] == ["--kernel-stats"]:
    name, path = argv[1], argv[2]
    with open(path) as f:
        rows = list(csv.DictReader(f))
    total = sum(float(r["TotalDurationNs"]) for r in rows) / 1e3 / REPS
    worst = max(rows, key=lambda r: float(r["TotalDurationNs"]))
    with open(OUT, "a") as f:
        f.write(f"kernel time per round, {name:<20} {total:10.1f} us  ({sum(int(r['Calls']) for r in rows) // REPS} launches; the "
                f"largest share: {worst['Name'][:60]})  [rocprofv3 --kernel-trace --stats, every kernel of a run of {REPS} "
                f"rounds / {REPS}]\n")
    sys.exit(0)

import torch

from golf_amd import functional as GF
from golf_amd.analysis_stream import GlottalSourceStream, ResidualStream, SpectralEnvelopeStream
from golf_amd.envelope import SpectralEnvelopeAnalysis
from golf_amd.glottal import GlottalSourceAnalysis
from golf_amd.lpc import LPCAnalysis
from golf_amd.synth import GlottalFlowTable


def inputs(device, seed=0):
    """Harmonic rows with noise and their f0 tracks in Hz: slow glides between 80 and 400 Hz, a third of the frames unvoiced
    (the signals of tools/time_hna_stream.py)."""
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
gain, a = LPCAnalysis(M, HOP).cuda().analyse(x)
env = SpectralEnvelopeAnalysis(SR, HOP, 1024, 240)
glo = GlottalSourceAnalysis(GlottalFlowTable(), SR, HOP).cuda()
e = GF.ltv_residual(x, gain, a, HOP)
blocks = [x[:, i:i + BLOCK] for i in range(0, T, BLOCK)]
e_blocks = [e[:, i:i + BLOCK] for i in range(0, T, BLOCK)]
n = len(blocks)


def late(t):   # the frames of the block before
    return [t[:, max(i - 1, 0) * PER:i * PER] for i in range(n)], t[:, (n - 1) * PER:]


f0_late, f0_rest = late(f0)
g_late, g_rest = late(gain)
a_late, a_rest = late(a)
env_st, res_st, glo_st = SpectralEnvelopeStream(env, B), ResidualStream(HOP, M, B), GlottalSourceStream(glo, B)


def fused():
    return GF.ltv_residual(x, gain, a, HOP)


def chain():
    num = GF.ltv_inverse(x, a, HOP)
    return num / GF.linear_upsample(gain, HOP)[:, :num.shape[1]]


def env_one_shot():
    return env(x, f0).as_tensor()


def env_stream():
    outs = [env_st.push(b, f).as_tensor() for b, f in zip(blocks, f0_late)]
    return outs + [env_st.push(f0=f0_rest).as_tensor(), env_st.finish().as_tensor()]


def res_stream():
    outs = [res_st.push(b, g, c) for b, g, c in zip(blocks, g_late, a_late)]
    return outs + [res_st.push(gain=g_rest, a=a_rest), res_st.finish()]


def glo_one_shot():
    return glo(e, f0).as_tensor()


def glo_stream():
    outs = [glo_st.push(b, f).as_tensor() for b, f in zip(e_blocks, f0_late)]
    return outs + [glo_st.push(f0=f0_rest).as_tensor(), glo_st.finish().as_tensor()]


VERSIONS = {"residual fused": fused, "residual chain": chain, "envelope one-shot": env_one_shot, "envelope stream": env_stream,
            "residual stream": res_stream, "glottal one-shot": glo_one_shot, "glottal stream": glo_stream}

if argv[:1] == ["--only"]:
    fn = VERSIONS[argv[1]]
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    sys.exit(0)

calls = {}
for one, st in (("envelope one-shot", "envelope stream"), ("residual fused", "residual stream"),
                ("glottal one-shot", "glottal stream")):
    outs = VERSIONS[st]()
    calls[st] = len(outs)
    assert torch.equal(torch.cat(outs, 1), VERSIONS[one]()), st
diff = (fused() - chain()).abs().max() / fused().abs().max()


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


for fn in VERSIONS.values():
    timed(fn, 3)
samples = {k: [] for k in VERSIONS}
for rep in range(5):
    for k, fn in VERSIONS.items():
        samples[k].append(timed(fn, REPS))
med = {k: statistics.median(s) for k, s in samples.items()}
# the bytes each residual version has to move: x in and e out, against the chain's three passes over (B, T) arrays
T_out = e.shape[1]
by_fused = 4 * (B * T + B * T_out + gain.numel() + a.numel())
by_chain = 4 * ((B * T + B * T_out + a.numel()) + (gain.numel() + B * ((F - 1) * HOP + 1)) + 3 * B * T_out)
with open(OUT, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: B={B} T={T} hop={HOP} M={M} ({B * F} frames); streams: {n} pushes of {BLOCK} "
            f"samples with the frame-rate input of the block before, the last frames, finish(); each stream equal to its "
            f"one-shot bit for bit; HIP events around whole rounds, 3 warm-up rounds, median of 5 windows ({REPS} rounds of each "
            f"version, alternating), us\n")
    for k in VERSIONS:
        per = f"   per call ({calls[k]} calls) {med[k] / calls[k]:8.1f}" if k in calls else ""
        f.write(f"{k:<20} {med[k]:10.1f}   (min {min(samples[k]):.1f}, max {max(samples[k]):.1f}){per}\n")
    f.write(f"residual: fused / chain call time {med['residual fused'] / med['residual chain']:.2f}; bytes the algorithm moves "
            f"{by_fused / 1e6:.1f} MB fused, {by_chain / 1e6:.1f} MB chain (ltv_inverse, linear_upsample, divide); largest "
            f"difference of the two results {float(diff):.2e} of the largest value (torch's interpolation weight)\n")
print(open(OUT).read())
