"""Device time of the source-compensated LPC analysis (golf_lpc_source_filter_f32, csrc/lpc_analysis.hip) at the recipe shape,
beside (a) the plain analysis' forward at the same shape (golf_lpc_analysis_fwd_f32: the same staging and lag passes for M
instead of M + Q lags and one recursion, so the difference is the cost of the added stages) and (b) the same definition
written with float64 torch ops on the same device (tests/sflpc_ref.py) (dev tool; bench.py is the contract).  Writes
profiles/sflpc_timing.txt, or the file given as the first argument.

B = 32, T = 48 000, W = 960, hop 240, M = 22, Q = 4, I = 2: 32 x 201 frames.  HIP events around INNER back-to-back calls
after a warm-up; the two HIP calls are timed in alternating rounds and the median of the rounds is reported with the
spread.  Also prints the worst per-frame differences to the float64 version, so that the times belong to results that
agree."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import sflpc_ref as R
from golf_amd import functional as GF

B, T, W, HOP, M, Q, I = 32, 48000, 960, 240, 22, 4, 2
OUT = os.path.join(ROOT, "profiles", "sflpc_timing.txt")


def timed_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def main():
    g = torch.Generator().manual_seed(2434)
    from scipy.signal import lfilter

    ex = torch.randn(B, T, generator=g, dtype=torch.float64).numpy()
    x = torch.tensor(lfilter([1.0, -0.9], [1.0, -1.6, 0.8], ex, axis=1)).float().cuda()   # a resonance and a tilt to find
    window = torch.hann_window(W).cuda()
    calls = {"hip source-filter (M + Q = 26 lags, 3 + 2 recursions)": lambda: GF.source_filter_lpc(x, window, HOP, M, Q, I),
             "hip plain lpc_analysis forward (22 lags, 1 recursion)": lambda: GF.lpc_analysis(x, window, HOP, M),
             "hip source-filter, iterations=0": lambda: GF.source_filter_lpc(x, window, HOP, M, Q, 0)}

    def torch_f64():
        return R.analysis(x, window, HOP, M, Q, I)

    with torch.no_grad():
        gain, a, rc, src = GF.source_filter_lpc(x, window, HOP, M, Q, I, return_rc=True, return_source=True)
        rgain, ra, rrc, rsrc = torch_f64()
        ea = ((a.double() - ra).abs().amax(-1) / ra.abs().amax(-1)).max().item()
        es = ((src.double() - rsrc).abs().amax(-1) / rsrc.abs().amax(-1)).max().item()
        erc = (rc.double() - rrc).abs().max().item()
        eg = ((gain.double() - rgain).abs() / rgain).max().item()
        for fn in calls.values():   # warm-up: code objects loaded, clocks up
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        rounds = {k: [] for k in calls}
        for _ in range(15):   # alternating rounds
            for k, fn in calls.items():
                rounds[k].append(timed_us(fn, 20))
        torch_f64()
        t_ref = sorted(timed_us(torch_f64, 1) for _ in range(5))
    med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
    names = list(calls)
    lines = [f"{torch.cuda.get_device_name(0)}: source_filter_lpc B={B} T={T} W={W} hop={HOP} M={M} Q={Q} I={I} "
             f"({B * (T // HOP + 1)} frames); HIP events, us per call: median of 15 alternating rounds of 20 calls (min .. max)",
             f"agreement with float64 torch: a {ea:.2e}  source {es:.2e} (worst frame, rel-max)  rc {erc:.2e}  gain {eg:.2e}"]
    lines += [f"{k:56s} {med[k]:10.1f}   ({min(rounds[k]):.1f} .. {max(rounds[k]):.1f})" for k in names]
    lines.append(f"{'torch float64 (tests/sflpc_ref.py), 5 calls':56s} {t_ref[2]:10.1f}   ({t_ref[0]:.1f} .. {t_ref[-1]:.1f})")
    lines.append(f"source-filter / plain forward: {med[names[0]] / med[names[1]]:.2f}   "
                 f"added by the stages: {med[names[0]] - med[names[1]]:.1f} us   "
                 f"torch float64 / source-filter: {t_ref[2] / med[names[0]]:.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
