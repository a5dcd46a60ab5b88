"""Device time of the minimum-phase FIR design (csrc/minphase_fir.hip) beside the zero-phase one (csrc/noise_fir.hip) in the
same process, of the causal frame FIR beside the zero-phase frame FIR, and of the whole filter (dev tool; bench.py is the
contract).  Writes profiles/minphase_fir_timing.txt.

G = B * F = 6400 rows, n_mag = 256 (the shipped noise-filter shape, B = 32, F = 200, hop 240, T = 48 000).  HIP events around
INNER back-to-back calls, warm-up, median of the repeats, the two filters alternating.

Work per row (multiply-adds on the matrix cores): minimum-phase forward 256*256 + 2*257*510 = 328 k, backward 393 k (with
theta recomputed); zero-phase 65.5 k each way: 5.0 x and 6.0 x.
Rule: design forward <= 8 x, design backward <= 10 x the zero-phase kernel's time (the margin is for exp / sincos and the
two-operand epilogue); the frame FIRs run the same core on the same arithmetic: parity expected.  Exit status 1 when the
design rule fails."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from golf_amd import _lib
from golf_amd import functional as GF

B, T, F, N_MAG, HOP = 32, 48000, 200, 256, 240
WARMUP, REPEATS, INNER = 5, 25, 10
OUT = os.path.join(ROOT, "profiles", "minphase_fir_timing.txt")


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / INNER)
    return sorted(times)[len(times) // 2]


def main():
    lib = _lib.load()
    g = torch.Generator().manual_seed(2434)
    N = 2 * (N_MAG - 1)
    G = B * F
    env = torch.cumsum(0.25 * torch.randn(B, 1, N_MAG, generator=g), 2) + torch.cumsum(0.05 * torch.randn(B, F, N_MAG, generator=g), 1)
    lm = (env - 2.0).clamp(-6, 3).cuda().contiguous()
    ex = torch.randn(B, T, generator=g).cuda()
    zwin = torch.hann_window(N).cuda()
    mwin = GF.min_phase_window(torch.hann_window, N, "cuda")
    zb, mb = GF.zero_phase_fir_basis(N_MAG, "cuda"), GF.min_phase_fir_basis(N_MAG, "cuda")
    KS = lib.golf_zero_phase_fir_row_stride(N_MAG)
    kern = torch.empty(G, KS, device="cuda")
    g_kern = torch.randn(G, KS, generator=g).cuda()
    g_lm = torch.empty_like(lm)
    st = _lib.stream_ptr()
    p = lambda t: t.data_ptr()
    chk = _lib.check

    calls = {
        "zp design fwd": lambda: chk(lib.golf_zero_phase_fir_kernels_f32(p(lm), p(zwin), p(zb), p(kern), G, N_MAG, st), "zp"),
        "mp design fwd": lambda: chk(lib.golf_min_phase_fir_kernels_f32(p(lm), p(mwin), p(mb), p(kern), G, N_MAG, st), "mp"),
        "zp design bwd": lambda: chk(lib.golf_zero_phase_fir_kernels_bwd_f32(p(g_kern), p(lm), p(zwin), p(zb), p(g_lm), G, N_MAG, st), "zpb"),
        "mp design bwd": lambda: chk(lib.golf_min_phase_fir_kernels_bwd_f32(p(g_kern), p(lm), p(mwin), p(mb), p(g_lm), G, N_MAG, st), "mpb"),
    }
    # frame FIRs on finished kernel rows
    zk = GF._fir_kernels_raw(GF.ZERO_PHASE_FIR, lm, zwin, zb)
    mk = GF._fir_kernels_raw(GF.MIN_PHASE_FIR, lm, mwin, mb)
    Tz, Tm = GF.fir_frames_length(T, F, N, HOP), GF.fir_frames_causal_length(T, F, N, HOP)
    yz, ym = torch.empty(B, Tz, device="cuda"), torch.empty(B, Tm, device="cuda")
    gz, gm = torch.randn(B, Tz, generator=g).cuda(), torch.randn(B, Tm, generator=g).cuda()
    g_ex, g_k = torch.empty_like(ex), torch.empty_like(zk)
    calls.update({
        "zp frames fwd": lambda: chk(lib.golf_ltv_fir_frames_fwd_f32(p(ex), T, p(zk), KS, p(yz), Tz, B, T, F, N, HOP, 0, st), "zf"),
        "mp frames fwd": lambda: chk(lib.golf_ltv_fir_frames_causal_fwd_f32(p(ex), T, p(mk), KS, p(ym), Tm, B, T, F, N, HOP, 0, st), "mf"),
        "zp frames bwd": lambda: chk(lib.golf_ltv_fir_frames_bwd_f32(p(gz), Tz, p(ex), T, p(zk), KS, p(g_ex), T, p(g_k), B, T, F, N, HOP, 0, st), "zfb"),
        "mp frames bwd": lambda: chk(lib.golf_ltv_fir_frames_causal_bwd_f32(p(gm), Tm, p(ex), T, p(mk), KS, p(g_ex), T, p(g_k), B, T, F, N, HOP, 0, st), "mfb"),
    })
    # whole filters through autograd
    exg, lmg = ex.clone().requires_grad_(True), lm.clone().requires_grad_(True)

    def whole(fn, win, gy, grad):
        def run():
            if not grad:
                with torch.no_grad():
                    fn(ex, lm, win, HOP)
                return
            exg.grad = lmg.grad = None
            fn(exg, lmg, win, HOP).backward(gy)
        return run

    calls.update({
        "zp filter fwd": whole(GF.zero_phase_fir_filter, zwin, gz, False),
        "mp filter fwd": whole(GF.min_phase_fir_filter, mwin, gm, False),
        "zp filter fwd+bwd": whole(GF.zero_phase_fir_filter, zwin, gz, True),
        "mp filter fwd+bwd": whole(GF.min_phase_fir_filter, mwin, gm, True),
    })
    t = {}
    for _ in range(2):   # two rounds, the filters alternating; the second one counts (everything warm)
        for name, fn in calls.items():
            t[name] = median_us(fn)
    lines = [f"{torch.cuda.get_device_name(0)}: B={B} T={T} F={F} n_mag={N_MAG} hop={HOP}  (G={G} rows, N={N} taps); "
             f"median of {REPEATS} x {INNER} calls, HIP events, us per call"]
    for what in ("design fwd", "design bwd", "frames fwd", "frames bwd", "filter fwd", "filter fwd+bwd"):
        z, m = t["zp " + what], t["mp " + what]
        lines.append(f"{what:15s} zero-phase {z:8.1f}   minimum-phase {m:8.1f}   ratio {m / z:5.2f}")
    macs_f, macs_b = G * (N_MAG * N_MAG + 2 * (N_MAG + 1) * N), G * (2 * N_MAG * N_MAG + 2 * (N_MAG + 1) * N)
    lines.append(f"design fwd {2e-6 * macs_f / t['mp design fwd']:.1f} TFLOP/s, bwd {2e-6 * macs_b / t['mp design bwd']:.1f} TFLOP/s "
                 f"(fp32 MFMA, multiply-adds of the algorithm x 2 over the time above)")
    rf, rb = t["mp design fwd"] / t["zp design fwd"], t["mp design bwd"] / t["zp design bwd"]
    ok = rf <= 8.0 and rb <= 10.0
    lines.append(f"rule design fwd <= 8 x: {rf:.2f} x {'PASS' if rf <= 8.0 else 'FAIL'}   design bwd <= 10 x: {rb:.2f} x "
                 f"{'PASS' if rb <= 10.0 else 'FAIL'}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
