"""Time of the spectral-envelope analysis (golf_spectral_envelope_f32, csrc/spec_envelope.hip) at B = 32 x 48 000 samples,
n_fft 1024, hop 240, 241 cepstral coefficients, with a mixed voiced / unvoiced f0 track between 80 and 400 Hz, next to a
stock-PyTorch restatement of the same definition on the same GPU, dev tool; bench.py is the contract.  Writes
profiles/env_timing.txt, or the file given as the first argument.

The restatement is what a user without the kernel would write: the frames gathered with the longest window and masks, the
window from float64 arguments, torch.fft.rfft (rocFFT) for the three transforms in fp32, the DC correction as a gather and
the smoothing as a difference of the float64 running integral of the evenly extended spectrum, in chunks of frames that fit
memory.  Three rows of both, the row where the two differ most among them, are checked against tests/env_ref.py (float64)
before anything is timed.  HIP events around back-to-back calls, 3 warm-up calls, the median of 5 windows with the two
variants alternating inside each round.  ``--cpu-check`` runs the restatement alone on the CPU at a tiny size against
tests/env_ref.py (no timing)."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

B, SR, HOP, N_FFT, N_CEPS, T = 32, 24000.0, 240, 1024, 241, 48000


def restatement(x, f0, sr, hop, n=N_FFT, n_ceps=N_CEPS, f0_floor=None, f0_ceil=None, unvoiced_f0=500.0, q1=-0.15, eps=1e-12,
                voiced_offset=0.5 * math.log(2.0), chunk=1024):
    """x (B, T), f0 (B, F) -> (log_env (B, F, n/2 + 1), ceps (B, F, n_ceps)): include/golf_amd.h in stock tensor ops."""
    f0_floor = 3.0 * sr / (n - 3) if f0_floor is None else f0_floor
    f0_ceil = sr / 12.0 if f0_ceil is None else f0_ceil
    (Bx, Tx), F = x.shape, f0.shape[1]
    dev, nh = x.device, n // 2
    fd = f0.double()
    v = fd > 0
    fe = torch.where(v, fd.clamp(f0_floor, f0_ceil), torch.full_like(fd, unvoiced_f0))
    G = Bx * F
    fe, v = fe.reshape(G, 1), v.reshape(G, 1)
    hw = torch.floor(1.5 * sr / fe + 0.5).long()
    r0 = fe * n / sr
    r = r0 / 3.0
    row = torch.arange(Bx, device=dev).repeat_interleave(F)[:, None]
    centre = (torch.arange(F, device=dev) * hop).repeat(Bx)[:, None]
    m = torch.arange(-(nh - 1), nh, device=dev)[None]                    # the longest window: n - 1 offsets
    k = torch.arange(nh + 1, device=dev, dtype=torch.float64)[None]
    zero64 = torch.zeros((), dtype=torch.float64, device=dev)
    log_env = torch.empty(G, nh + 1, device=dev)
    ceps = torch.empty(G, n_ceps, device=dev)
    for g0 in range(0, G, chunk):
        sl = slice(g0, min(g0 + chunk, G))
        fc, hc, r0c, rc = fe[sl], hw[sl], r0[sl], r[sl]
        mask = m.abs() <= hc
        w = torch.where(mask, 0.5 + 0.5 * torch.cos(2 * math.pi * m * fc / (3.0 * sr)), zero64).float()
        t = centre[sl] + m
        ok = mask & (t >= 0) & (t < Tx)
        xs = torch.where(ok, x[row[sl], t.clamp(0, max(Tx - 1, 0))], torch.zeros((), device=dev))
        xw = w * xs
        xw = xw - w * (xw.sum(1, keepdim=True) / w.sum(1, keepdim=True))
        buf = torch.zeros(xw.shape[0], n, device=dev)
        buf[:, m[0] % n] = xw
        X = torch.fft.rfft(buf, dim=1)
        P = (X.real ** 2 + X.imag ** 2) / (w * w).sum(1, keepdim=True)
        # DC correction
        u = r0c - k
        low = u > 0
        i0 = torch.floor(u).clamp(0, nh).long()
        tt = (u - i0).float()
        rep = (1 - tt) * P.gather(1, i0) + tt * P.gather(1, (i0 + 1).clamp(max=nh))
        Pc = torch.where(low, P + rep, P)
        # smoothing: the running integral of the even extension (cells -nh .. 2 nh) in float64, read at k - r and k + r
        ext = torch.cat([Pc[:, 1:].flip(1), Pc, Pc[:, :-1].flip(1)], 1).double()      # cell j at index j + nh
        I = torch.nn.functional.pad(torch.cumsum(ext, 1), (1, 0))                      # I[i]: the integral up to j - 1/2, j = i - nh

        def integral(tp):
            pos = tp + 0.5 + nh
            i = torch.floor(pos).long()
            return I.gather(1, i) + (pos - i) * ext.gather(1, i)

        Ps = ((integral(k + rc) - integral(k - rc)) / (2 * rc)).float()
        L = torch.log(Ps + eps)
        c = torch.fft.irfft(L, n=n, dim=1)[:, : nh + 1]
        tq = fc * k / sr
        lift = (torch.sinc(tq) * ((1 - 2 * q1) + 2 * q1 * torch.cos(2 * math.pi * tq))).float()
        cl = c * lift
        off = torch.where(v[sl], voiced_offset, 0.0).float()
        sym = torch.cat([cl, cl[:, 1:-1].flip(1)], 1)
        log_env[sl] = 0.5 * torch.fft.rfft(sym, dim=1).real + off
        cp = 0.5 * cl[:, :n_ceps]
        cp[:, :1] += off
        ceps[sl] = cp
    return log_env.reshape(Bx, F, nh + 1), ceps.reshape(Bx, F, n_ceps)


def inputs(device, Bn=B, Tn=T, seed=0):
    """Harmonic rows with noise and their f0 tracks in Hz: slow glides between 80 and 400 Hz, a third of the frames unvoiced."""
    g = torch.Generator().manual_seed(seed)
    F = Tn // HOP + 1
    lo = 95.0 * (345.0 / 95.0) ** torch.rand(Bn, 1, generator=g)
    f0 = lo * (1 + 0.15 * torch.sin(torch.arange(F) * 0.05 + 6.28 * torch.rand(Bn, 1, generator=g)))
    up = torch.nn.functional.interpolate(f0[:, None], size=(F - 1) * HOP + 1, mode="linear", align_corners=True)[:, 0]
    ph = torch.cumsum(up.double() / SR, 1)[:, :Tn]
    x = sum(torch.sin(2 * math.pi * h * ph) / h for h in range(1, 25)).float() * 0.3 + 0.05 * torch.randn(Bn, Tn, generator=g)
    unvoiced = (torch.arange(F)[None] // 10 + torch.arange(Bn)[:, None]) % 3 == 0
    return x.to(device), torch.where(unvoiced, torch.zeros(()), f0).float().to(device)


sys.path.insert(0, os.path.join(ROOT, "tests"))
import env_ref as R


def against_ref(env, ceps, ref):
    return R.errors(dict(log_env=env.double().cpu().numpy(), ceps=ceps.double().cpu().numpy()), ref)


if "--cpu-check" in sys.argv:
    x, f0 = inputs("cpu", 2, 2400, 1)
    env, ceps = restatement(x, f0, SR, HOP, chunk=7)
    ref = R.analyse(x.numpy(), f0.numpy(), SR, HOP, n_ceps=N_CEPS)
    print("restatement against tests/env_ref.py: magnitudes %.2e of the frame's largest, ceps %.2e Np" % against_ref(env, ceps, ref))
    sys.exit(0)

from golf_amd import functional as GF

x, f0 = inputs("cuda")
F = f0.shape[1]
hip = lambda: GF.spectral_envelope(x, f0, SR, HOP, N_FFT, n_ceps=N_CEPS)
stock = lambda: restatement(x, f0, SR, HOP)
(e1, c1), (e2, c2) = hip(), stock()
apart = (e1 - e2).abs().amax((1, 2))
ROWS = sorted({0, 13, int(apart.argmax())})
ref = R.analyse(x[ROWS].cpu().numpy(), f0[ROWS].cpu().numpy(), SR, HOP, n_ceps=N_CEPS)
against = {"hip": against_ref(e1[ROWS], c1[ROWS], ref), "stock": against_ref(e2[ROWS], c2[ROWS], ref)}
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
out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else os.path.join(ROOT, "profiles", "env_timing.txt")
with open(out, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: spectral_envelope B={B} T={T} hop={HOP} n_fft={N_FFT} n_ceps={N_CEPS} ({B * F} "
            f"frames, {voiced} voiced, f0 80..400 Hz); HIP events around back-to-back calls, 3 warm-up calls, median of 5 windows "
            "(20 hip calls, 2 stock calls each, alternating), us per call\n")
    f.write(f"largest difference between the two: log_env {float(apart.max()):.2e} Np (row {int(apart.argmax())})\n")
    for name, (e_env, e_ceps) in against.items():
        f.write(f"{name} against tests/env_ref.py (float64), rows {ROWS}, {len(ROWS) * F} frames: magnitudes {e_env:.2e} of the "
                f"frame's largest, ceps {e_ceps:.2e} Np\n")
    f.write(f"hip spectral_envelope                 {med['hip']:10.1f}   (min {min(samples['hip']):.1f}, max {max(samples['hip']):.1f})\n")
    f.write(f"stock PyTorch (gather, masks, rocFFT) {med['stock']:10.1f}   (min {min(samples['stock']):.1f}, max {max(samples['stock']):.1f})\n")
    f.write(f"stock / hip: {med['stock'] / med['hip']:.1f}\n")
print(open(out).read())
