"""Device time per frame-sample of the frame-wise filter OFF the ring grid (wave-per-frame kernels, csrc/lpc_ff_any.hip)
beside the ring chain (csrc/lpc_ff.hip) in the same process (dev tool; bench.py is the contract).

B = 32, F = 201, hop 240, W = 960, Tx = 48 000 (nfr = 201 frames).  HIP events, warm-up, median of the repeats; forward and
backward (= forward + backward - forward) in ns per frame-sample: time / (B * nfr * W).

Gated pair:    M = 38 (ring chain: the quad kernels)  vs  M = 40 (wave-per-frame kernels).
Rule: new <= 3 x ring, for the forward and for the backward separately.  Exit status 1 when it fails.
Reported pair: the backward at M = 22 with W = 1000 (ring forward, wave-per-frame adjoint and g_a) beside W = 960 (ring)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from golf_amd import functional as GF
from golf_amd.synthetic import make_inputs

B, F, HOP, TX = 32, 201, 240, 48000
WARMUP, REPEATS = 3, 15
FACTOR = 3.0


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return sorted(times)[len(times) // 2]


def measure(M, W):
    inp = make_inputs(B=B, T=F * HOP, hop=HOP, M=M, device="cuda")
    ex, gain, a = inp["noise"][:, :TX].contiguous(), inp["gain"][:, :F].contiguous(), inp["a"][:, :F].contiguous()
    win = torch.hann_window(W, device="cuda")
    _, nfr, Ty = GF.ff_output_length(TX, F, HOP, W)
    gy = torch.randn(B, Ty, device="cuda")
    exg, gg, ag = (t.clone().requires_grad_(True) for t in (ex, gain, a))

    def fwd():
        with torch.no_grad():
            GF.lti_frames_ola(ex, gain, a, win, HOP)

    def fwd_bwd():
        exg.grad = gg.grad = ag.grad = None
        GF.lti_frames_ola(exg, gg, ag, win, HOP).backward(gy)

    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    n = B * nfr * W
    return nfr, t_f * 1e6 / n, t_fb * 1e6 / n


def line(tag, M, W, nfr, f, fb):
    print(f"{tag:<34s} M={M:2d} W={W:4d} nfr={nfr}:  fwd {f:7.4f} ns/frame-sample ({f * B * nfr * W * 1e-3:7.1f} us)   "
          f"fwd+bwd {fb:7.4f}   bwd {fb - f:7.4f} ({(fb - f) * B * nfr * W * 1e-3:7.1f} us)")


def main():
    assert GF.ff_on_ring_grid(38, HOP, 960, backward=True) and not GF.ff_on_ring_grid(40, HOP)
    assert GF.ff_on_ring_grid(22, HOP, 960, backward=True) and not GF.ff_on_ring_grid(22, HOP, 1000, backward=True)
    print(f"B={B} F={F} hop={HOP} Tx={TX}   (median of {REPEATS}, HIP events)")
    nfr, f_on, fb_on = measure(38, 960)
    line("ring chain", 38, 960, nfr, f_on, fb_on)
    nfr, f_off, fb_off = measure(40, 960)
    line("wave per frame", 40, 960, nfr, f_off, fb_off)
    b_on, b_off = fb_on - f_on, fb_off - f_off
    ok_f, ok_b = f_off <= FACTOR * f_on, b_off <= FACTOR * b_on
    print(f"rule new <= {FACTOR:g} x ring:  fwd {f_off / f_on:.2f} x {'PASS' if ok_f else 'FAIL'}   "
          f"bwd {b_off / b_on:.2f} x {'PASS' if ok_b else 'FAIL'}")
    print("reported, not gated:")
    nfr, f, fb = measure(22, 960)
    line("ring chain", 22, 960, nfr, f, fb)
    nfr, f, fb = measure(22, 1000)
    line("ring forward, wave-per-frame bwd", 22, 1000, nfr, f, fb)
    return 0 if ok_f and ok_b else 1


if __name__ == "__main__":
    sys.exit(main())
