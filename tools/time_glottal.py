"""Time of the glottal-source match (golf_glottal_match_f32, csrc/glottal_match.hip) alone at B = 32 x 48 000 samples, hop 240
(6 432 frames), the package's 100-row table, 64 harmonics, 256 phase shifts, next to a stock-PyTorch restatement of the search
on the same GPU, dev tool; bench.py is the contract.  Writes profiles/glottal_timing.txt, or the file given as the first
argument.

The inputs are the harmonics (functional.harmonic_analysis, not timed) of pulses from the package's own oscillator on glides
between 90 and 350 Hz with a random-walk table position, a sixth of the frames unvoiced.  The restatement is what a user
without the kernel would write: per chunk of frames D = c conj(S) as (frames, K, 2 H) fp32, one batched matrix product with
the (2 H, n_phi) cosines and sines (rocBLAS), the division by sqrt(N[k, Hf] E2) and an argmax over K n_phi scores; it stops
at the grid (k*, j*), without the two refinements.  Its grid result is checked against the kernel's before anything is timed.
HIP events around back-to-back calls, 3 warm-up calls, the median of 5 windows with the two variants alternating inside each
round; the restatement's peak memory is torch's allocator peak over one call.  ``--cpu-check`` runs the restatement alone on
the CPU at a tiny size against tests/glottal_ref.py (no timing)."""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

B, SR, HOP, T, H, N_PHI = 32, 24000.0, 240, 48000, 64, 256


def restatement(amp, ph, f0, S, N, sr, n_phi, chunk=512):
    """amp, ph (B, F, H), f0 (B, F), the plan's S (K, H, 2) and N (K, H) -> (k*, j*, rho[k*, j*]), (B, F) each; k* = -1
    where there is no estimate."""
    (Bx, F, Hx), K, dev = amp.shape, S.shape[0], amp.device
    G = Bx * F
    ang = 2 * math.pi * (ph.reshape(G, Hx).double() - 0.25)
    a = amp.reshape(G, Hx)
    h = torch.arange(1, Hx + 1, device=dev)
    live = (h * (f0.reshape(G, 1).double() / sr) < 0.5) & (f0.reshape(G, 1) > 0)
    a = torch.where(live, a, torch.zeros((), device=dev))
    cr, ci = a * torch.cos(ang).float(), a * torch.sin(ang).float()
    Hf = live.sum(1)
    E2 = (a.double() ** 2).sum(1)
    ok = (Hf > 0) & (E2 > 0)
    hj = (h[:, None] * torch.arange(n_phi, device=dev)[None]) % n_phi
    arg = 2 * math.pi * hj.double() / n_phi
    trig = torch.cat([torch.cos(arg), torch.sin(arg)], 0).float()                       # (2 H, n_phi)
    Sr, Si = S[..., 0][None], S[..., 1][None]
    nk = N.double()[:, (Hf - 1).clamp(min=0)].T                                         # (G, K)
    inv = torch.where(nk > 0, (nk * E2[:, None]).clamp(min=1e-300).rsqrt(), torch.zeros((), dtype=torch.float64, device=dev)).float()
    ks = torch.full((G,), -1, dtype=torch.long, device=dev)
    js = torch.zeros(G, dtype=torch.long, device=dev)
    best = torch.zeros(G, device=dev)
    for g0 in range(0, G, chunk):
        sl = slice(g0, min(g0 + chunk, G))
        r, i = cr[sl, None], ci[sl, None]
        D = torch.cat([r * Sr + i * Si, i * Sr - r * Si], 2)                            # (g, K, 2 H)
        rho = torch.matmul(D, trig) * inv[sl, :, None]                                  # (g, K, n_phi)
        v, flat = rho.reshape(rho.shape[0], -1).max(1)
        ks[sl], js[sl], best[sl] = flat // n_phi, flat % n_phi, v
    ks = torch.where(ok, ks, torch.full_like(ks, -1))
    return ks.reshape(Bx, F), js.reshape(Bx, F), torch.where(ok, best, torch.zeros_like(best)).reshape(Bx, F)


if "--cpu-check" in sys.argv:
    import glottal_ref as R

    c = R.cases()["recipe"]
    amp, ph = R.harmonics(c)
    S, N, X = R.plan(c["table"], c["H"])
    ref = R.match(amp, ph, c["f0"], S, N, X, c["sample_rate"], c["n_phi"])
    ks, js, rho = restatement(torch.tensor(amp), torch.tensor(ph), torch.tensor(c["f0"]), torch.tensor(S), torch.tensor(N),
                              c["sample_rate"], c["n_phi"], chunk=7)
    ok = ks.numpy() >= 0
    assert (ok == ~(ref["w"] != ref["w"])).all()
    print("restatement against tests/glottal_ref.py: k* differs in %d, j* in %d of %d frames" % (
        (ks.numpy() != ref["k"])[ok].sum(), (js.numpy() != ref["j"])[ok].sum(), ok.sum()))
    sys.exit(0)

from golf_amd import functional as GF
from golf_amd.audiotensor import AudioTensor
from golf_amd.synth import IndexedGlottalFlowTable

g = torch.Generator().manual_seed(0)
F = T // HOP + 1
lo = 90.0 * (300.0 / 90.0) ** torch.rand(B, 1, generator=g)
f0 = (lo * (1 + 0.15 * torch.sin(torch.arange(F) * 0.05 + 6.28 * torch.rand(B, 1, generator=g)))).float().cuda()
w = (0.1 + 0.8 * torch.rand(B, 1, generator=g) + torch.cumsum(0.01 * torch.randn(B, F, generator=g), 1)).clamp(0.05, 0.95).cuda()
osc = IndexedGlottalFlowTable(oversampling=4).cuda()
e = osc(AudioTensor(f0 / SR, HOP), AudioTensor(w, HOP)).as_tensor()
e = e + 0.01 * e.std() * torch.randn(e.shape, generator=g).cuda()
unvoiced = ((torch.arange(F)[None] // 10 + torch.arange(B)[:, None]) % 6 == 0).cuda()
f0 = torch.where(unvoiced, torch.zeros((), device="cuda"), f0)
amp, ph = GF.harmonic_analysis(e, f0, SR, HOP, H, return_phases=True)
plan = GF.glottal_plan(osc.table, H)
K = plan.spectrum.shape[0]
hip = lambda: GF.glottal_match(amp, ph, f0, plan, SR, N_PHI)
stock = lambda: restatement(amp, ph, f0, plan.spectrum, plan.norms, SR, N_PHI)
(w1, th1, rho1), (ks, js, rho2) = hip(), stock()
has = ks >= 0
assert bool((torch.isnan(w1) == ~has).all())
dw = ((w1 * (K - 1) - ks)[has]).abs().max()
dth = (th1 - js / N_PHI)[has].abs()
dth = torch.minimum(dth, 1 - dth).max() * N_PHI
drho = (rho1 - rho2)[has]
torch.cuda.reset_peak_memory_stats()
base = torch.cuda.memory_allocated()
stock()
torch.cuda.synchronize()
peak = torch.cuda.max_memory_allocated() - base


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
    samples["hip"].append(timed(hip, 50))
    samples["stock"].append(timed(stock, 3))
med = {k: statistics.median(s) for k, s in samples.items()}
flop = 4.0 * int(has.sum()) * K * H * N_PHI
out = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else os.path.join(ROOT, "profiles", "glottal_timing.txt")
with open(out, "w") as f:
    f.write(f"{torch.cuda.get_device_name(0)}: glottal_match B={B} T={T} hop={HOP} ({B * F} frames, {int(has.sum())} with an "
            f"estimate) K={K} H={H} n_phi={N_PHI}; HIP events around back-to-back calls, 3 warm-up calls, median of 5 windows "
            "(50 hip calls, 3 stock calls each, alternating), us per call\n")
    f.write(f"the two agree: kernel w within {float(dw):.2f} rows of the grid k*, theta within {float(dth):.2f} columns of the "
            f"grid j*, refined rho - grid rho in [{float(drho.min()):.1e}, {float(drho.max()):.1e}]\n")
    f.write(f"hip glottal_match (one launch)            {med['hip']:10.1f}   (min {min(samples['hip']):.1f}, max {max(samples['hip']):.1f})"
            f"   {flop / med['hip'] * 1e-6:.1f} TFLOP/s of the {flop * 1e-9:.1f} GFLOP the scores take\n")
    f.write(f"stock PyTorch (chunks of 512, matmul, max) {med['stock']:9.1f}   (min {min(samples['stock']):.1f}, max {max(samples['stock']):.1f})\n")
    f.write(f"stock / hip: {med['stock'] / med['hip']:.1f}\n")
    f.write(f"stock PyTorch peak memory over one call: {peak / 2 ** 20:.0f} MiB (the kernel allocates its three (B, F) outputs)\n")
print(open(out).read())
