"""Device time of the sample-wise filter from an initial state (functional.ltv_allpole_ss(zi=...), csrc/lpc_state.hip) beside
the plain call in the same process (dev tool; bench.py is the contract and runs zi=None).

B = 32, M = 22, hop 240, F = 201 (T = 48 001).  HIP events, 3 warm-up calls, median of 15:
  * forward and forward + backward of the plain call -- the code path without the feature, the baseline;
  * forward and forward + backward of the same call with zi (return_zf=True, a cotangent on zf as well);
  * a torch copy_ of a (B, T) fp32 tensor: one read and one write of the bytes that the head moves.
The head adds one read and one write of (B, T) to the forward (one extra launch, plus the fill of the all-ones gain) and two
reads and one write to the backward (two extra launches), so the added time is set beside 1 x and 1.5 x the copy."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from golf_amd import functional as GF
from golf_amd.synthetic import make_inputs

B, M, HOP, F = 32, 22, 240, 201
WARMUP, REPEATS = 3, 15


def median_us(fn):
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
        times.append(e0.elapsed_time(e1) * 1e3)
    return sorted(times)[len(times) // 2]


def main():
    T = (F - 1) * HOP + 1
    inp = make_inputs(B=B, T=F * HOP, hop=HOP, M=M, device="cuda")
    ex, gain, a = inp["noise"][:, :T].contiguous(), inp["gain"][:, :F].contiguous(), inp["a"][:, :F].contiguous()
    zi = 0.3 * torch.randn(B, M, device="cuda")
    gy, gzf = torch.randn(B, T, device="cuda"), torch.randn(B, M, device="cuda")
    exg, gg, ag, zg = (t.clone().requires_grad_(True) for t in (ex, gain, a, zi))
    src, dst = torch.randn(B, T, device="cuda"), torch.empty(B, T, device="cuda")

    def fwd():
        with torch.no_grad():
            GF.ltv_allpole_ss(ex, gain, a, HOP)

    def fwd_zi():
        with torch.no_grad():
            GF.ltv_allpole_ss(ex, gain, a, HOP, zi=zi, return_zf=True)

    def fwd_bwd():
        exg.grad = gg.grad = ag.grad = None
        GF.ltv_allpole_ss(exg, gg, ag, HOP).backward(gy)

    def fwd_bwd_zi():
        exg.grad = gg.grad = ag.grad = zg.grad = None
        y, zf = GF.ltv_allpole_ss(exg, gg, ag, HOP, zi=zg, return_zf=True)
        torch.autograd.backward((y, zf), (gy, gzf))

    t_copy = median_us(lambda: dst.copy_(src))
    t_f, t_fz = median_us(fwd), median_us(fwd_zi)
    t_fb, t_fbz = median_us(fwd_bwd), median_us(fwd_bwd_zi)
    t_f2, t_fz2 = median_us(fwd), median_us(fwd_zi)   # (a second pass over the forward pair: the spread of the figure)
    nbytes = 2 * B * T * 4
    print(f"B={B} M={M} hop={HOP} F={F} T={T}   (median of {REPEATS}, HIP events, us)")
    print(f"copy_ of (B, T) fp32:        {t_copy:8.1f}   ({nbytes / t_copy / 1e6:.2f} TB/s read + write)")
    print(f"forward       plain {t_f:8.1f}   with zi {t_fz:8.1f}   added {t_fz - t_f:7.1f}   (again: {t_f2:.1f} / {t_fz2:.1f})")
    print(f"fwd+backward  plain {t_fb:8.1f}   with zi {t_fbz:8.1f}   added {t_fbz - t_fb:7.1f}")
    print(f"backward      plain {t_fb - t_f:8.1f}   with zi {t_fbz - t_fz:8.1f}   added {(t_fbz - t_fz) - (t_fb - t_f):7.1f}")
    print(f"bytes at the copy rate: forward 1.0 x copy = {t_copy:.1f}, backward 1.5 x copy = {1.5 * t_copy:.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
