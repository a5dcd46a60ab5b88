"""Time of the harmonic-plus-noise analysis (golf_harmonic_analysis_f32, csrc/harm_analysis.hip) at B = 32 x 48 000 samples,
hop 240, K = 155, n_mag = 256 with a mixed voiced / unvoiced f0 track between 80 and 400 Hz, next to a stock-PyTorch
restatement of the same definition on the same GPU, dev tool; bench.py is the contract.  Writes profiles/hna_timing.txt, or
the file given as the first argument.

The restatement is what a user without the kernel would write: the frames batched with a fixed max_window and masks, the
phases k phi(m) in float64 (mod 1) and everything after them in fp32 tensor ops (complex matrix products), in chunks of frames
that fit memory.  Three rows of both, the row where the two differ most among them, are checked against tests/hna_ref.py
(float64) before anything is timed.  HIP events around back-to-back calls, 3 warm-up calls, the median of 5 windows with the two
variants alternating inside each round.  ``--cpu-check`` runs the
restatement alone on the CPU at a tiny size against tests/hna_ref.py (no timing)."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

B, SR, HOP, K, N_MAG, T = 32, 24000.0, 240, 155, 256, 48000


def restatement(x, f0, sr, hop, K, n_mag, periods=4, min_window=None, max_window=2048, unvoiced_window=None, eps=1e-12,
                chunk=96):
    """x (B, T), f0 (B, F) -> (amplitudes (B, F, K), log_mag (B, F, n_mag)): include/golf_amd.h in stock tensor ops."""
    min_window = 2 * hop if min_window is None else min_window
    unvoiced_window = 4 * hop if unvoiced_window is None else unvoiced_window
    (Bx, Tx), F = x.shape, f0.shape[1]
    dev = x.device
    fd = f0.double()
    v = fd > 0
    safe = torch.where(v, fd, torch.ones_like(fd))
    n_per = torch.clamp(torch.ceil(min_window * safe / sr), min=periods)
    L = torch.where(v, torch.clamp(torch.floor(n_per * sr / safe + 0.5), 2, max_window), torch.full_like(fd, unvoiced_window))
    prev = torch.nn.functional.pad(fd[:, :-1], (1, 0))
    nxt = torch.nn.functional.pad(fd[:, 1:], (0, 1))
    pv, nv = prev > 0, nxt > 0
    s = torch.where(pv & nv, (nxt - prev) / (2 * hop * sr),
                    torch.where(nv, (nxt - fd) / (hop * sr), torch.where(pv, (fd - prev) / (hop * sr), torch.zeros_like(fd))))
    omega = fd / sr
    G = Bx * F
    L, s, omega, v = L.reshape(G, 1).long(), s.reshape(G, 1), omega.reshape(G, 1), v.reshape(G, 1)
    row = torch.arange(Bx, device=dev).repeat_interleave(F)[:, None]
    centre = (torch.arange(F, device=dev) * hop).repeat(Bx)[:, None]
    i = torch.arange(max_window, device=dev)[None]
    ks = torch.arange(1, K + 1, device=dev, dtype=torch.float64)
    bs = torch.arange(n_mag, device=dev, dtype=torch.float64)
    amp = torch.empty(G, K, device=dev)
    log_mag = torch.empty(G, n_mag, device=dev)
    for g0 in range(0, G, chunk):
        sl = slice(g0, min(g0 + chunk, G))
        Lc, vc = L[sl], v[sl]
        mask = i < Lc
        m = i - Lc // 2
        w = torch.where(mask, 0.5 - 0.5 * torch.cos(2 * math.pi * (i + 0.5) / Lc), torch.zeros((), dtype=torch.float64, device=dev))
        t = centre[sl] + m
        ok = mask & (t >= 0) & (t < Tx)
        xs = torch.where(ok, x[row[sl], t.clamp(0, Tx - 1)], torch.zeros((), device=dev))
        w32 = w.float()
        wx = (w32 * xs).to(torch.complex64)
        md = m.double()
        phi = omega[sl] * md + s[sl] * md * md / 2
        th = torch.remainder(ks[None, :, None] * phi[:, None, :], 1.0).float()
        E = torch.polar(torch.ones_like(th), -2 * math.pi * th)                      # (g, K, W)
        c = torch.bmm(E, wx[:, :, None])[:, :, 0] * (2.0 / w.sum(1, keepdim=True)).float()
        c = torch.where((ks[None] * omega[sl] < 0.5) & vc, c, torch.zeros((), dtype=torch.complex64, device=dev))
        amp[sl] = c.abs()
        model = torch.bmm(c.conj()[:, None, :], E)[:, 0, :].real
        r = xs - model
        tb = torch.remainder(bs[None, :, None] * md[:, None, :] / (2 * (n_mag - 1)), 1.0).float()
        En = torch.polar(torch.ones_like(tb), -2 * math.pi * tb)                     # (g, n_mag, W)
        z = torch.bmm(En, (w32 * r).to(torch.complex64)[:, :, None])[:, :, 0]
        S = (z.real.double() ** 2 + z.imag.double() ** 2) / (w * w).sum(1, keepdim=True)
        log_mag[sl] = (0.5 * torch.log(S + eps)).float()
    return amp.reshape(Bx, F, K), log_mag.reshape(Bx, F, n_mag)


def inputs(device, Bn=B, Tn=T, seed=0):
    """Harmonic rows with noise and their f0 tracks in Hz: slow glides between 80 and 400 Hz, a third of the frames unvoiced."""
    g = torch.Generator().manual_seed(seed)
    F = Tn // HOP + 1
    lo = 95.0 * (345.0 / 95.0) ** torch.rand(Bn, 1, generator=g)   # 80.75 .. 396.75 Hz with the vibrato: no harmonic sits on Nyquist
    f0 = lo * (1 + 0.15 * torch.sin(torch.arange(F) * 0.05 + 6.28 * torch.rand(Bn, 1, generator=g)))
    up = torch.nn.functional.interpolate(f0[:, None], size=(F - 1) * HOP + 1, mode="linear", align_corners=True)[:, 0]
    ph = torch.cumsum(up.double() / SR, 1)[:, :Tn]
    x = sum(torch.sin(2 * math.pi * h * ph) / h for h in range(1, 25)).float() * 0.3 + 0.05 * torch.randn(Bn, Tn, generator=g)
    unvoiced = (torch.arange(F)[None] // 10 + torch.arange(Bn)[:, None]) % 3 == 0
    return x.to(device), torch.where(unvoiced, torch.zeros(()), f0).float().to(device)


if "--cpu-check" in sys.argv:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hna_ref as R

    x, f0 = inputs("cpu", 2, 2400, 1)
    a, lm = restatement(x, f0, SR, HOP, 20, 33, chunk=7)
    ref = R.analyse(x.numpy(), f0.numpy(), SR, HOP, 20, 33)
    print("restatement against tests/hna_ref.py: amp %.2e, magnitude %.2e" % (
        (a.double() - torch.tensor(ref["amp"])).abs().max(), (lm.double().exp() - torch.tensor(ref["log_mag"]).exp()).abs().max()))
    sys.exit(0)

from golf_amd import functional as GF

x, f0 = inputs("cuda")
F = f0.shape[1]
hip = lambda: GF.harmonic_analysis(x, f0, SR, HOP, K, n_mag=N_MAG)
stock = lambda: restatement(x, f0, SR, HOP, K, N_MAG)
(a1, l1), (a2, l2) = hip(), stock()
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hna_ref as R

# each against the float64 oracle on three rows, the one where the two differ most among them: the largest error per frame in
# units of the frame's scale (max |x| over its window)
apart = (a1 - a2).abs().amax((1, 2))
ROWS = sorted({0, 13, int(apart.argmax())})
ref = R.analyse(x[ROWS].cpu().numpy(), f0[ROWS].cpu().numpy(), SR, HOP, K, N_MAG)
against = {}
for name, (a, l) in (("hip", (a1, l1)), ("stock", (a2, l2))):
    got = dict(amp=a[ROWS].double().cpu().numpy(), log_mag=l[ROWS].double().cpu().numpy(), phase=ref["phase"])
    against[name] = R.errors(got, ref)[:2]
voiced = int((f0 > 0).sum())


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


for fn in (hip, stock):
    timed(fn, 3)
samples = {"hip": [], "stock": []}
for rep in range(5):
    samples["hip"].append(timed(hip, 20))
    samples["stock"].append(timed(stock, 2))
med = {k: statistics.median(s) for k, s in samples.items()}
out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else os.path.join(ROOT, "profiles", "hna_timing.txt")
with open(out, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: harmonic_analysis B={B} T={T} hop={HOP} K={K} n_mag={N_MAG} ({B * F} frames, "
            f"{voiced} voiced, f0 80..400 Hz); HIP events around back-to-back calls, 3 warm-up calls, median of 5 windows "
            "(20 hip calls, 2 stock calls each, alternating), us per call\n")
    f.write(f"largest difference between the two: amplitudes {float(apart.max()):.2e} (row {int(apart.argmax())})\n")
    for name, (e_amp, e_mag) in against.items():
        f.write(f"{name} against tests/hna_ref.py (float64), rows {ROWS}, {len(ROWS) * F} frames: amplitudes {e_amp:.2e}, magnitudes {e_mag:.2e} "
                "of the frame's scale\n")
    f.write(f"hip harmonic_analysis                 {med['hip']:10.1f}   (min {min(samples['hip']):.1f}, max {max(samples['hip']):.1f})\n")
    f.write(f"stock PyTorch (fp32 complex bmm)      {med['stock']:10.1f}   (min {min(samples['stock']):.1f}, max {max(samples['stock']):.1f})\n")
    f.write(f"stock / hip: {med['stock'] / med['hip']:.1f}\n")
print(open(out).read())
