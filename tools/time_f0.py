"""Device time of the f0 analysis (csrc/f0_yin.hip) at the recipe shape beside a stock-PyTorch rendering of the same
definition on the same device: unfolded frames, the cross-correlation of the difference function d[tau] = e(0) + e(tau) -
2 r(tau) on rocFFT, running energies by cumsum, then cumsum, search and refinement in tensor ops, all fp32 (dev tool;
bench.py is the contract).  Writes profiles/f0_yin_timing.txt, or the file given as the first argument.

B = 32, T = 48 000, hop 240, W = 1024, 60 - 1000 Hz at 24 kHz (lags 24 .. 400): 32 x 201 frames.  HIP events around one call,
three warm-up calls, median of 15, the two alternating in one process.  Both are checked against tests/f0_ref.py (float64)
on the first rows, so that the times belong to results that agree.  The kernel's VALU issue bound is computed from the shapes:
one packed subtract and one packed fused multiply-add per two lag products, four cycles per wave instruction."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import f0_ref as R
from golf_amd import functional as GF

B, T, SR, HOP, W, F0_MIN, F0_MAX, THETA = 32, 48000, 24000.0, 240, 1024, 60.0, 1000.0, 0.15
CHECK_ROWS = 4
OUT = os.path.join(ROOT, "profiles", "f0_yin_timing.txt")


def torch_yin(x, tau_min, tau_max):
    """The definition in stock tensor ops, fp32: (f0, period, ap)."""
    S = W + tau_max
    n_fft = 1 << (S - 1).bit_length()
    s = torch.nn.functional.pad(x, (S // 2, S - S // 2)).unfold(1, S, HOP)[:, : T // HOP + 1]          # (B, F, S)
    r = torch.fft.irfft(torch.fft.rfft(s[..., :W], n_fft).conj() * torch.fft.rfft(s, n_fft), n_fft)[..., : tau_max + 1]
    c = torch.nn.functional.pad(torch.cumsum(s * s, -1), (1, 0))
    e = c[..., W:W + tau_max + 1] - c[..., : tau_max + 1]                                                # e(tau)
    d = (e[..., :1] + e - 2 * r).clamp_min(0)
    run = torch.cumsum(d[..., 1:], -1)
    tau = torch.arange(1, tau_max + 1, device=x.device, dtype=x.dtype)
    dp = torch.cat([torch.ones_like(d[..., :1]), torch.where(run != 0, d[..., 1:] * tau / run, torch.ones_like(run))], -1)
    idx = torch.arange(tau_max + 1, device=x.device)
    in_range = idx >= tau_min
    below = (dp < THETA) & in_range
    found = below.any(-1)
    first = torch.where(found, below.int().argmax(-1), torch.zeros_like(found, dtype=torch.long))
    nxt = torch.nn.functional.pad(dp[..., 1:], (0, 1), value=float("inf"))
    stop = ~(nxt < dp) & (idx >= first[..., None])               # the descent ends here; always true at tau_max
    walked = stop.int().argmax(-1)
    lowest = torch.where(in_range, dp, torch.full_like(dp, float("inf"))).argmin(-1)
    star = torch.where(found, walked, lowest)
    a, b, c3 = (dp.gather(-1, (star + k).clamp(0, tau_max)[..., None])[..., 0] for k in (-1, 0, 1))
    den = a - 2 * b + c3
    inner = (star - 1 >= 1) & (star + 1 <= tau_max) & (den > 0)
    delta = torch.where(inner, ((a - c3) / (2 * den.where(inner, torch.ones_like(den)))).clamp(-1, 1), torch.zeros_like(den))
    period = star + delta
    ap = b - (a - c3) * delta / 4
    voiced = found & (e[..., 0] > 0)
    return torch.where(voiced, SR / period, torch.zeros_like(period)), period, ap


def agreement(out, ref):
    f0, period, ap = (t[:CHECK_ROWS].double().cpu().numpy() for t in out)
    flips = (np.abs(period - ref["tau"]) > 1) | ((f0 > 0) != ref["voiced"])
    ok = ~flips
    return (f"{int(flips.sum())} of {flips.size} frames differ in lag or voicing; on the rest period "
            f"{(np.abs(period - ref['period']) / ref['period'])[ok].max():.2e} relative, ap {np.abs(ap - ref['ap'])[ok].max():.2e} absolute")


def main():
    tau_min, tau_max, _ = GF.f0_lags(SR, F0_MIN, F0_MAX, W)
    rng = np.random.default_rng(1424)
    rows = []
    for b in range(B):   # glides between random pitches in a little noise, every fourth row noise alone
        g = R.glide(rng.uniform(80, 400), rng.uniform(80, 400), T, SR, 8)[0]
        rows.append(rng.normal(0, 1, T) if b % 4 == 3 else g + 0.05 * rng.normal(0, 1, T))
    x_host = np.array(rows).astype(np.float32)
    x = torch.tensor(x_host).cuda()
    ref = R.yin(x_host[:CHECK_ROWS], SR, HOP, W, tau_min, tau_max, THETA)

    def hip():
        return GF.f0_yin(x, SR, HOP, F0_MIN, F0_MAX, W, THETA, return_all=True)

    def stock():
        return torch_yin(x, tau_min, tau_max)

    with torch.no_grad():
        checks = [agreement(hip(), ref), agreement(stock(), ref)]
        for _ in range(3):
            hip(), stock()
        torch.cuda.synchronize()
        times = {"hip": [], "torch": []}
        for _ in range(15):
            for name, fn in (("hip", hip), ("torch", stock)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        burst = []   # ten calls back to back: the device time of a call once the host's part of it is hidden
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                hip()
            e1.record()
            torch.cuda.synchronize()
            burst.append(e0.elapsed_time(e1) * 1e2)
    t_hip, t_torch, t_burst = sorted(times["hip"])[7], sorted(times["torch"])[7], sorted(burst)[2]
    prop = torch.cuda.get_device_properties(0)
    frames = B * (T // HOP + 1)
    products = frames * (tau_max + 1) * W
    simds, mhz = prop.multi_processor_count * 4, getattr(prop, "clock_rate", 2400000) / 1e3
    bound = products / 64 * 4 / (simds * mhz)   # one packed instruction per product and lane, 4 cycles each
    lines = [f"{torch.cuda.get_device_name(0)}: f0_yin B={B} T={T} hop={HOP} W={W} lags {tau_min}..{tau_max} ({frames} frames, "
             f"{products / 1e9:.2f} G lag products); HIP events, median of 15 after 3 warm-up calls, us per call",
             f"hip kernel against tests/f0_ref.py (float64), {CHECK_ROWS} rows: {checks[0]}",
             f"torch fp32 rendering against the same: {checks[1]}",
             f"{'hip f0_yin':28s} {t_hip:12.1f}   (min {min(times['hip']):.1f})",
             f"{'torch fp32 (rocFFT, tensor ops)':28s} {t_torch:12.1f}   (min {min(times['torch']):.1f})",
             f"torch / hip: {t_torch / t_hip:.2f}",
             f"VALU issue bound of the kernel, packed fp32 ({simds} SIMDs at {mhz:.0f} MHz): {bound:.1f} us; "
             f"a call is at {100 * bound / t_hip:.0f} % of it",
             f"ten hip calls back to back (the host's share of a call hidden), median of 5: {t_burst:.1f} us per call, "
             f"{100 * bound / t_burst:.0f} % of the bound"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
