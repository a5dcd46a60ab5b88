"""Device time of the LPC analysis (csrc/lpc_analysis.hip) at the recipe shape, forward and forward + backward, beside the
same definition written with float64 torch ops on the same device (tests/lpc_analysis_ref.py: unfold, one product-sum per
lag, the recursion as a Python loop) -- the only composition of torch ops that meets the 1e-4 parity bar (dev tool; bench.py
is the contract).  Writes profiles/lpc_analysis_timing.txt, or the file given as the first argument.

B = 32, T = 48 000, W = 960, hop 240, M = 22: 32 x 201 frames.  HIP events around INNER back-to-back calls after a warm-up,
median of the repeats.  Also prints the worst per-frame differences between the two, so that the times belong to results
that agree."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import lpc_analysis_ref as R
from golf_amd import functional as GF

B, T, W, HOP, M = 32, 48000, 960, 240, 22
OUT = os.path.join(ROOT, "profiles", "lpc_analysis_timing.txt")


def median_us(fn, warmup, repeats, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / inner)
    return sorted(times)[len(times) // 2]


def main():
    g = torch.Generator().manual_seed(2434)
    from scipy.signal import lfilter

    ex = torch.randn(B, T, generator=g, dtype=torch.float64).numpy()
    x = torch.tensor(lfilter([1.0], [1.0, -1.6, 0.8], ex, axis=1)).float().cuda()   # a two-pole resonance for the recursion to find
    window = torch.hann_window(W).cuda()
    xg = x.clone().requires_grad_(True)
    xd = x.double().requires_grad_(True)
    cot = [torch.randn(B, T // HOP + 1, generator=g).cuda(), torch.randn(B, T // HOP + 1, M, generator=g).cuda()]

    def hip_fwd():
        with torch.no_grad():
            return GF.lpc_analysis(x, window, HOP, M)

    def hip_fwd_bwd():
        xg.grad = None
        gain, a = GF.lpc_analysis(xg, window, HOP, M)
        torch.autograd.backward([gain, a], cot)

    def torch_fwd():
        with torch.no_grad():
            return R.analysis(x, window, HOP, M)[:2]

    def torch_fwd_bwd():
        xd.grad = None
        gain, a, _ = R.analysis(xd, window, HOP, M)
        torch.autograd.backward([gain, a], [c.double() for c in cot])

    gain, a = hip_fwd()
    rgain, ra = torch_fwd()
    hip_fwd_bwd()
    torch_fwd_bwd()
    ea = ((a.double() - ra).abs().amax(-1) / ra.abs().amax(-1)).max().item()
    eg = ((gain.double() - rgain).abs() / rgain).max().item()
    egx = ((xg.grad.double() - xd.grad).abs().max() / xd.grad.abs().max()).item()
    t = {"hip fwd": median_us(hip_fwd, 5, 15, 10), "hip fwd+bwd": median_us(hip_fwd_bwd, 5, 15, 10),
         "torch float64 fwd": median_us(torch_fwd, 1, 5, 1), "torch float64 fwd+bwd": median_us(torch_fwd_bwd, 1, 5, 1)}
    lines = [f"{torch.cuda.get_device_name(0)}: lpc_analysis B={B} T={T} W={W} hop={HOP} M={M} ({B * (T // HOP + 1)} frames); "
             f"HIP events, median, us per call",
             f"agreement of the two: a {ea:.2e} (worst frame, rel-max)  gain {eg:.2e}  g_x {egx:.2e}"]
    lines += [f"{k:24s} {v:12.1f}" for k, v in t.items()]
    lines.append(f"fp64 multiply-adds of the lags: {B * (T // HOP + 1) * (M + 1) * W / 1e6:.0f} M")
    # the gather walks about (256 + W) / hop frames per 256-sample tile: the same signal at small hops (4 rows)
    for w2, h2 in ((960, 240), (960, 16), (1024, 4), (4096, 1)):
        x4, win2 = xg[:4].detach().clone().requires_grad_(True), torch.hann_window(w2).cuda()
        f2 = T // h2 + 1
        cot2 = [torch.randn(4, f2, generator=g).cuda(), torch.randn(4, f2, M, generator=g).cuda()]

        def fwd2():
            with torch.no_grad():
                GF.lpc_analysis(x4, win2, h2, M)

        def both2():
            x4.grad = None
            torch.autograd.backward(list(GF.lpc_analysis(x4, win2, h2, M)), cot2)

        tf, tb = median_us(fwd2, 2, 5, 2), median_us(both2, 2, 5, 2)
        lines.append(f"B=4 W={w2:5d} hop={h2:4d} ({4 * f2:7d} frames, {(256 + w2) // h2 + 1:5d} frames per gather tile): "
                     f"fwd {tf:10.1f}   fwd+bwd {tb:10.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
