"""Device time per sample of the sample-wise filter's float64 recursion beside the fp32 instantiation of the same
wave-per-utterance kernels (csrc/lpc_any.hip), in one process (dev tool; bench.py is the contract).  Reported, not gated.

B = 32 x 48 001 samples, M = 22:  hop 240 through the float64 recursion -- fp32 tensors with mode="fp64" (io = fp32) and
float64 tensors (io = fp64) -- and hop 300 (off the ring grid) through the fp32 chain.  All three run one recursion per
utterance from t = 0 to T.  The timing method of tools/time_anyshape.py: HIP events, warm-up, median of the repeats; forward
and backward (= forward + backward - forward) in ns per sample (time / T)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from golf_amd import functional as GF
from golf_amd.synthetic import make_inputs
from time_anyshape import REPEATS, median_ms

B, M, T = 32, 22, 48001


def measure(hop, dtype, mode):
    F = (T - 1) // hop + 1
    inp = make_inputs(B=B, T=F * hop, hop=hop, M=M, device="cuda")
    ex, gain, a = (inp[k][:, :n].contiguous().to(dtype) for k, n in (("noise", T), ("gain", F), ("a", F)))
    gy = torch.randn(B, T, device="cuda", dtype=dtype)
    exg, gg, ag = (t.clone().requires_grad_(True) for t in (ex, gain, a))

    def fwd():
        with torch.no_grad():
            GF.ltv_allpole_ss(ex, gain, a, hop, mode=mode)

    def fwd_bwd():
        exg.grad = gg.grad = ag.grad = None
        GF.ltv_allpole_ss(exg, gg, ag, hop, mode=mode).backward(gy)

    t_f, t_fb = median_ms(fwd), median_ms(fwd_bwd)
    return t_f * 1e6 / T, (t_fb - t_f) * 1e6 / T


def main():
    assert not GF.ss_is_trainable(M, 300, 161) and GF.ss_has_f64(M, 240, 201)
    rows = [("fp32 chain  hop 300 (lpc_any.hip)", measure(300, torch.float32, None)),
            ("float64     hop 240 io = fp32    ", measure(240, torch.float32, "fp64")),
            ("float64     hop 240 io = fp64    ", measure(240, torch.float64, None)),
            ("float64     hop 300 io = fp32    ", measure(300, torch.float32, "fp64"))]
    f0, b0 = rows[0][1]
    print(f"B={B} M={M} T={T}   (median of {REPEATS}, HIP events; ns per sample = time / T)")
    for name, (f, b) in rows:
        print(f"{name}:  fwd {f:7.2f} ns/sample ({f / f0:4.2f} x)   bwd {b:7.2f} ({b / b0:4.2f} x)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
