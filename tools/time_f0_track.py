"""Device time of the f0 tracker at the recipe shape: golf_f0_yin_f32 (unchanged, the yardstick of the candidate kernel), the
candidate kernel (csrc/f0_yin.hip), the path kernel (csrc/f0_viterbi.hip) and a stock-PyTorch rendering of the same path
recursion on the same device, the four alternating in one process (dev tool; bench.py is the contract).  Writes
profiles/f0_track_timing.txt, or the file given as the first argument.

B = 32, T = 48 000, hop 240, W = 1024, 60 - 1000 Hz at 24 kHz (lags 24 .. 400), K = 7: 32 x 201 frames.  HIP events around one
call, three warm-up calls, median of 15; and ten path calls replayed from one graph.  The stock rendering is what a user has without the kernel: local and transition
costs of every frame in a few batched float64 tensor ops, then one (add, min over `from`, add) per frame and one gather per
frame on the way back -- F dependent steps of a few tiny launches each.  f0_yin and the candidates are checked against
tests/f0_ref.py and tests/f0_track_ref.py (float64) on the first rows, the kernel's path against the reference's path on the kernel's own
candidates, and the stock rendering's path against the kernel's on every row.  Exit status 1 only if the path kernel is not
faster than the stock rendering."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import f0_ref as R
import f0_track_ref as TR
from golf_amd import functional as GF

B, T, SR, HOP, W, F0_MIN, F0_MAX, K = 32, 48000, 24000.0, 240, 1024, 60.0, 1000.0, 7
CHECK_ROWS = 2
OUT = os.path.join(ROOT, "profiles", "f0_track_timing.txt")


def torch_path(p, a, lag_ref, unvoiced_cost, lag_cost, jump_cost, switch_cost):
    """The path recursion in stock tensor ops, float64: (f0, state)."""
    Bn, F, Kn = p.shape
    p64, a64 = p.double(), a.double()
    inf = float("inf")
    pres = (p64 > 0) & (a64 < inf)                                                       # false for NaN and +inf
    lp = torch.log2(torch.where(pres, p64, torch.ones_like(p64)))
    voiced = torch.where(pres, a64.clamp_min(0) + lag_cost * (lp - math.log2(lag_ref)), torch.full_like(a64, inf))
    loc = torch.cat([torch.full_like(voiced[..., :1], unvoiced_cost), voiced], -1)       # (B, F, 1 + K)
    lp = torch.cat([torch.zeros_like(lp[..., :1]), lp], -1)
    pres = torch.cat([torch.ones_like(pres[..., :1]), pres], -1)
    t = jump_cost * (lp[:, 1:, None, :] - lp[:, :-1, :, None]).abs()                      # (B, F - 1, from, to)
    t[:, :, 0, :] = switch_cost
    t[:, :, :, 0] = switch_cost
    t[:, :, 0, 0] = 0.0
    t = torch.where(pres[:, :-1, :, None] & pres[:, 1:, None, :], t, torch.full_like(t, inf))
    C = loc[:, 0]
    back = []
    for f in range(1, F):
        v, i = (C[:, :, None] + t[:, f - 1]).min(1)
        C = loc[:, f] + v
        back.append(i)
    s = C.argmin(-1)
    states = [s]
    for i in reversed(back):
        s = i.gather(1, s[:, None])[:, 0]
        states.append(s)
    state = torch.stack(states[::-1], 1)
    period = p64.gather(2, (state - 1).clamp_min(0)[..., None])[..., 0]
    f0 = torch.where(state > 0, SR / period.where(state > 0, torch.ones_like(period)), torch.zeros_like(period))
    return f0.float(), state.int()


def main():
    tau_min, tau_max, _ = GF.f0_lags(SR, F0_MIN, F0_MAX, W)
    rng = np.random.default_rng(1424)
    rows = []
    for b in range(B):   # glides between random pitches in a little noise, every fourth row noise alone
        g = R.glide(rng.uniform(80, 400), rng.uniform(80, 400), T, SR, 8)[0]
        rows.append(rng.normal(0, 1, T) if b % 4 == 3 else g + 0.05 * rng.normal(0, 1, T))
    x_host = np.array(rows).astype(np.float32)
    x = torch.tensor(x_host).cuda()
    costs = GF.F0_VITERBI_COSTS

    def yin():
        return GF.f0_yin(x, SR, HOP, F0_MIN, F0_MAX, W, return_all=True)

    def cand():
        return GF.f0_candidates(x, SR, HOP, F0_MIN, F0_MAX, W, K)

    with torch.no_grad():
        cp, ca = cand()

        def path():
            return GF.f0_viterbi(cp, ca, SR, float(tau_min), return_state=True, **costs)

        def stock():
            return torch_path(cp, ca, float(tau_min), **costs)

        # checks, so that the times belong to results that agree
        ref = TR.candidates(x_host[:CHECK_ROWS], SR, HOP, W, tau_min, tau_max, K)
        gp, ga = (t[:CHECK_ROWS].double().cpu().numpy() for t in (cp, ca))
        there = ref["lag"] >= 0
        flips = (((gp > 0) != there) | (there & (np.abs(gp - ref["lag"]) > 1))).any(-1)
        ok = ~flips[..., None] & there
        check_c = (f"{int(flips.sum())} of {flips.size} frames differ in their lags; on the rest period "
                   f"{(np.abs(gp[ok] - ref['period'][ok]) / ref['period'][ok]).max():.2e} relative, "
                   f"ap {np.abs(ga[ok] - ref['ap'][ok]).max():.2e} absolute")
        y = tuple(t[:CHECK_ROWS].double().cpu().numpy() for t in yin())
        yflips = (np.abs(y[1] - ref["yin"]["tau"]) > 1) | ((y[0] > 0) != ref["yin"]["voiced"])
        check_y = (f"{int(yflips.sum())} of {yflips.size} frames differ in lag or voicing; on the rest period "
                   f"{(np.abs(y[1] - ref['yin']['period']) / ref['yin']['period'])[~yflips].max():.2e} relative")
        f0_hip, st_hip = path()
        own = TR.viterbi(cp[:CHECK_ROWS].cpu().numpy(), ca[:CHECK_ROWS].cpu().numpy(), SR, float(tau_min), **costs)
        diff_ref = int((st_hip[:CHECK_ROWS].cpu().numpy() != own["state"]).sum())
        check_p = f"{diff_ref} of {own['state'].size} states differ (reference margin {own['margin']:.2e})"
        f0_t, st_t = stock()
        diff_t = int((st_t != st_hip).sum())
        check_t = (f"{diff_t} of {st_hip.numel()} states differ from the kernel's; f0 within "
                   f"{float((f0_t - f0_hip)[st_t == st_hip].abs().max()):.2e} Hz on the rest")
        voiced = float((st_hip > 0).float().mean())

        fns = (("yin", yin), ("cand", cand), ("path", path), ("torch", stock))
        for _ in range(3):
            for _, fn in fns:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in fns}
        for _ in range(15):
            for name, fn in fns:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        # the path kernel's own device time: ten calls captured in one graph, so that no host work sits between them
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(10):
                path()
        burst = []
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graph.replay()
            e1.record()
            torch.cuda.synchronize()
            burst.append(e0.elapsed_time(e1) * 1e2)
        burst = burst[1:]
    med = {name: sorted(v)[7] for name, v in times.items()}
    frames = T // HOP + 1
    lines = [f"{torch.cuda.get_device_name(0)}: f0 tracker B={B} T={T} hop={HOP} W={W} lags {tau_min}..{tau_max} K={K} ({B} x {frames} "
             f"frames, {100 * voiced:.0f} % of them voiced on the path); HIP events, median of 15 after 3 warm-up calls, us per call",
             f"f0_yin against tests/f0_ref.py (float64), {CHECK_ROWS} rows: {check_y}",
             f"candidate kernel against tests/f0_track_ref.py (float64), {CHECK_ROWS} rows: {check_c}",
             f"path kernel against the reference on the kernel's candidates, {CHECK_ROWS} rows: {check_p}",
             f"torch float64 rendering of the path: {check_t}",
             f"{'hip f0_yin (unchanged)':34s} {med['yin']:12.1f}   (min {min(times['yin']):.1f})",
             f"{'hip f0_candidates':34s} {med['cand']:12.1f}   (min {min(times['cand']):.1f})",
             f"{'hip f0_viterbi':34s} {med['path']:12.1f}   (min {min(times['path']):.1f})",
             f"{'torch float64 path (tensor ops)':34s} {med['torch']:12.1f}   (min {min(times['torch']):.1f})",
             f"candidates / yin: {med['cand'] / med['yin']:.2f}",
             f"torch path / hip path: {med['torch'] / med['path']:.1f}",
             f"ten hip path calls replayed from one captured graph (no host work between them), median of 5: "
             f"{sorted(burst)[2]:.1f} us per call, {sorted(burst)[2] * 1e3 / frames:.0f} ns per frame"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0 if med["path"] < med["torch"] else 1


if __name__ == "__main__":
    sys.exit(main())
