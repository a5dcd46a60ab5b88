"""Device time per sample of the sample-wise filter OFF the ring grid (wave-per-utterance kernels, csrc/lpc_any.hip) beside
the ring path's serial kernels in the same process (dev tool; bench.py is the contract).

B = 32, M = 22, F = 161:  hop 300 (off the grid, T = 48 001)  vs  hop 240 with mode="serial" (on the grid, T = 38 401) -- the
same arithmetic per sample, and both run one recursion per utterance from t = 0 to T.  HIP events, warm-up, median of the
repeats; forward and backward (= forward + backward - forward) in ns per sample (time / T).

Rule: off-grid ns per sample <= 2 x the on-grid serial figure, for the forward and for the backward separately.  Exit status 1
when it fails."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from golf_amd import functional as GF
from golf_amd.synthetic import make_inputs

B, M, F = 32, 22, 161
WARMUP, REPEATS = 3, 15
FACTOR = 2.0


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


def measure(hop, mode):
    T = (F - 1) * hop + 1
    inp = make_inputs(B=B, T=F * hop, hop=hop, M=M, device="cuda")
    ex, gain, a = inp["noise"][:, :T].contiguous(), inp["gain"][:, :F].contiguous(), inp["a"][:, :F].contiguous()
    gy = torch.randn(B, T, device="cuda")
    exg, gg, ag = (t.clone().requires_grad_(True) for t in (ex, gain, a))

    def fwd():
        with torch.no_grad():
            GF.ltv_allpole_ss(ex, gain, a, hop, mode=mode)

    def fwd_bwd():
        exg.grad = gg.grad = ag.grad = None
        GF.ltv_allpole_ss(exg, gg, ag, hop, mode=mode).backward(gy)

    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    return T, t_f * 1e6 / T, t_fb * 1e6 / T


def main():
    assert GF.ss_is_trainable(M, 240, F) and not GF.ss_is_trainable(M, 300, F)
    T_on, f_on, fb_on = measure(240, "serial")
    T_off, f_off, fb_off = measure(300, None)
    b_on, b_off = fb_on - f_on, fb_off - f_off
    print(f"B={B} M={M} F={F}   (median of {REPEATS}, HIP events)")
    print(f"on grid   hop 240 serial  T={T_on}:  fwd {f_on:7.2f} ns/sample   fwd+bwd {fb_on:7.2f}   bwd {b_on:7.2f}")
    print(f"off grid  hop 300         T={T_off}:  fwd {f_off:7.2f} ns/sample   fwd+bwd {fb_off:7.2f}   bwd {b_off:7.2f}")
    ok_f, ok_b = f_off <= FACTOR * f_on, b_off <= FACTOR * b_on
    print(f"rule off <= {FACTOR:g} x on:  fwd {f_off / f_on:.2f} x {'PASS' if ok_f else 'FAIL'}   "
          f"bwd {b_off / b_on:.2f} x {'PASS' if ok_b else 'FAIL'}")
    return 0 if ok_f and ok_b else 1


if __name__ == "__main__":
    sys.exit(main())
