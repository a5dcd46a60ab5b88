"""Device time of the mel-cepstral design kernel (csrc/mlsa_design.hip) beside the named torch composition of the same rows
(functional.mel_cepstrum_response_torch, its cosine / sine tables built once outside the timed calls) in the same process, and
of the whole LTVMLSAFilter2 on either (dev tool; bench.py is the contract).  Writes profiles/mlsa_design_timing.txt.

B = 32, F = 201, M = 24, n_fft = 1024, alpha 0.46, hop 240, T = 48 000: R = 6432 rows of 513 complex bins, 26.4 MB.  HIP
events around INNER back-to-back calls, the two sides alternating repeat by repeat after warm-up, median of the repeats
(REPEATS x INNER = 150 calls a side).

Counted per call: the kernel writes the rows once (26.4 MB) and reads 0.64 MB of mel cepstra; 2 x 25 x 513 multiply-adds a
row, 0.33 GFLOP.  The torch composition makes at least five row-sized passes (two products, the negation, the complex pair,
the exponential) and keeps activations for the backward.
Rule: the kernel path is not slower than the torch composition on rows forward and on rows forward + backward.  Exit status 1
when it is."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from golf_amd import functional as GF
from golf_amd.audiotensor import AudioTensor
from golf_amd.filters import LTVMLSAFilter2

B, T, F, M, N, ALPHA, HOP = 32, 48000, 201, 24, 1024, 0.46, 240
WARMUP, REPEATS, INNER = 5, 15, 10
OUT = os.path.join(ROOT, "profiles", "mlsa_design_timing.txt")


def window_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / INNER


def pair_us(kernel_fn, torch_fn):
    for _ in range(WARMUP):
        kernel_fn(), torch_fn()
    torch.cuda.synchronize()
    tk, tt = [], []
    for _ in range(REPEATS):
        tk.append(window_us(kernel_fn))
        tt.append(window_us(torch_fn))
    med = lambda v: sorted(v)[len(v) // 2]
    return med(tk), med(tt), (min(tk), max(tk)), (min(tt), max(tt))


def main():
    g = torch.Generator().manual_seed(2434)
    K = N // 2 + 1
    mc = torch.randn(B, F, M + 1, generator=g) * 0.5 * 0.8 ** torch.arange(M + 1)
    mc[..., 0] = torch.empty(B, F).uniform_(-1, 1, generator=g)
    mc = mc.cuda()
    g_h = torch.complex(torch.randn(B, F, K, generator=g), torch.randn(B, F, K, generator=g)).cuda()
    ex = torch.randn(B, T, generator=g).cuda()
    basis = GF.mel_cepstrum_basis(N, M, ALPHA, "cuda")
    tables = GF.mel_cepstrum_tables(N, M, ALPHA, torch.float32, "cuda")
    mcg = mc.clone().requires_grad_(True)
    exg = ex.clone().requires_grad_(True)
    flt = LTVMLSAFilter2(N, HOP, M, alpha=ALPHA).cuda()
    with torch.no_grad():
        gy = torch.randn_like(flt(AudioTensor(ex), AudioTensor(mc, HOP)).as_tensor())
        err = (GF.mel_cepstrum_rows(mc, basis, N) - GF.mel_cepstrum_response_torch(mc, N, ALPHA, tables)).abs().max()

    def rows_fwd_kernel():
        GF.mel_cepstrum_rows(mc, basis, N)

    def rows_fwd_torch():
        with torch.no_grad():
            GF.mel_cepstrum_response_torch(mc, N, ALPHA, tables)

    def rows_train_kernel():
        mcg.grad = None
        GF.mel_cepstrum_response(mcg, N, ALPHA, basis=basis).backward(g_h)

    def rows_train_torch():
        mcg.grad = None
        GF.mel_cepstrum_response_torch(mcg, N, ALPHA, tables).backward(g_h)

    kernel_rows = GF.mel_cepstrum_response

    def module(rows):
        def run():
            GF.mel_cepstrum_response = rows     # what LTVMLSAFilter2.response_rows calls
            try:
                mcg.grad = exg.grad = None
                flt(AudioTensor(exg), AudioTensor(mcg, HOP)).as_tensor().backward(gy)
            finally:
                GF.mel_cepstrum_response = kernel_rows
        return run

    torch_rows = lambda m, n_fft, alpha, basis=None: GF.mel_cepstrum_response_torch(m, n_fft, alpha, tables)
    pairs = (("rows fwd", rows_fwd_kernel, rows_fwd_torch), ("rows fwd+bwd", rows_train_kernel, rows_train_torch),
             ("filter fwd+bwd", module(kernel_rows), module(torch_rows)))
    R = B * F
    lines = [f"{torch.cuda.get_device_name(0)}: B={B} F={F} M={M} n_fft={N} alpha={ALPHA} hop={HOP} T={T}  (R={R} rows x {K} bins, "
             f"{R * K * 8 / 1e6:.1f} MB); median of {REPEATS} x {INNER} calls a side, alternating, HIP events, us per call",
             f"max |kernel rows - torch rows| = {float(err):.2e}"]
    t = {}
    for name, kf, tf in pairs:
        k, c, ks, cs = t[name] = pair_us(kf, tf)
        lines.append(f"{name:15s} kernel {k:8.1f} ({ks[0]:.1f} .. {ks[1]:.1f})   torch composition {c:8.1f} ({cs[0]:.1f} .. {cs[1]:.1f})"
                     f"   torch / kernel {c / k:5.2f}")
    k = t["rows fwd"][0]
    lines.append(f"rows fwd: {R * K * 8 / k / 1e6:.2f} TB/s of rows written, {2e-6 * 2 * (M + 1) * K * R / k:.2f} TFLOP/s "
                 "(bytes and multiply-adds of the algorithm over the time above)")
    ok = all(t[n][0] <= t[n][1] for n in ("rows fwd", "rows fwd+bwd"))
    lines.append("rule kernel <= torch composition on rows fwd and rows fwd+bwd: " + ("PASS" if ok else "FAIL"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
