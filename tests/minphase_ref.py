"""Float64 restatement of the minimum-phase FIR filter (TEST INFRASTRUCTURE; torch on the CPU, autograd for the gradients).

The design is the dense form of the reference's get_minimum_phase_fir (models/filters.py:203-214 with hilbert,
models/utils.py:557-574).  With N = 2*(n_mag-1) and w_k = 1 for k in {0, N/2}, 2 otherwise:

    c[n]     = (1/N) sum_{k<=N/2} w_k L[k] cos(2 pi k n / N)                 n = 0..N/2   (real cepstrum)
    theta[k] = - sum_{n<=N/2} w_n c[n] sin(2 pi k n / N)                     k = 0..N/2
    h[m]     = (1/N) sum_{k<=N/2} w_k e^{L[k]} cos(theta[k] + 2 pi k m / N)  m = 0..N-1

The matrices are built from these sums as written (no closed form), with integer argument reduction.  The filters are
    frame-wise:  y[b, f*hop+n] = sum_{j<N} h[b,f,j] ex[b, f*hop+n-j],            T // hop frames
    sample-wise: y[b, t] = sum_j ((1-w_t) h[b,f,j] + w_t h[b,f+1,j]) ex[b, t-j],  f = t // hop, w_t = (t % hop) / hop,
                 t < min(T, (F-1)*hop+1)
tests/test_minphase_host.py pins all of it to the reference's own output (tests/golden/g29) at 1e-12."""
import functools

import numpy as np
import torch


@functools.lru_cache(maxsize=None)
def design_matrices(n_mag: int):
    """(Ccep (n_mag, n_mag): c = L @ Ccep.T;  Sth (n_mag, n_mag): theta = c @ Sth.T;  cosine and sine synthesis (n_mag, N))."""
    N = 2 * (n_mag - 1)
    k = np.arange(n_mag)
    w = np.where((k == 0) | (k == N // 2), 1.0, 2.0)
    ang = lambda a, b: 2.0 * np.pi * (np.outer(a, b) % N) / N
    Ccep = np.cos(ang(k, k)) * w[None, :] / N                  # [n, k]
    Sth = -np.sin(ang(k, k)) * w[None, :]                      # [k, n]
    m = np.arange(N)
    Cs = np.cos(ang(k, m)) * w[:, None] / N                    # [k, m]
    Ss = np.sin(ang(k, m)) * w[:, None] / N
    return tuple(torch.from_numpy(x) for x in (Ccep, Sth, Cs, Ss))


def min_phase_window(name: str, N: int) -> torch.Tensor:
    fn = {"hanning": torch.hann_window, "hamming": torch.hamming_window}[name]
    w = fn(N, dtype=torch.float64)
    w[: N // 2] = 1
    return w


def min_phase_kernels(log_mag: torch.Tensor, window: torch.Tensor = None) -> torch.Tensor:
    """(..., n_mag) float64 -> (..., N) minimum-phase impulse responses, times ``window`` if given."""
    Ccep, Sth, Cs, Ss = design_matrices(log_mag.shape[-1])
    theta = (log_mag @ Ccep.T) @ Sth.T
    mag = torch.exp(log_mag)
    h = (mag * torch.cos(theta)) @ Cs - (mag * torch.sin(theta)) @ Ss
    return h if window is None else h * window


def causal_frames(ex: torch.Tensor, h: torch.Tensor, hop: int) -> torch.Tensor:
    """ex (B,T), h (B,F,N) -> (B, (T // hop) * hop)."""
    B, T = ex.shape
    N = h.shape[-1]
    nfr = T // hop
    assert 1 <= nfr <= h.shape[1]
    xp = torch.nn.functional.pad(ex, (N - 1, 0))
    y = ex.new_zeros(B, nfr, hop)
    for j in range(N):   # xp[N-1 + t - j] = ex[t - j]
        y = y + h[:, :nfr, j: j + 1] * xp[:, N - 1 - j: N - 1 - j + nfr * hop].reshape(B, nfr, hop)
    return y.reshape(B, nfr * hop)


def causal_samplewise(ex: torch.Tensor, h: torch.Tensor, hop: int) -> torch.Tensor:
    """ex (B,T), h (B,F,N) -> (B, min(T, (F-1)*hop+1)): the kernels linearly interpolated to sample rate."""
    B, T = ex.shape
    F, N = h.shape[1], h.shape[2]
    Tout = min(T, (F - 1) * hop + 1)
    t = torch.arange(Tout)
    f, w = t // hop, ((t % hop).to(torch.float64) / hop)[None, :, None]
    f1 = torch.clamp(f + 1, max=F - 1)
    ht = (1 - w) * h[:, f] + w * h[:, f1]                     # (B, Tout, N)
    xp = torch.nn.functional.pad(ex, (N - 1, 0))
    y = ex.new_zeros(B, Tout)
    for j in range(N):
        y = y + ht[:, :, j] * xp[:, N - 1 - j: N - 1 - j + Tout]
    return y


def filter_with_grads(ex, log_mag, window, hop: int, gy=None, samplewise: bool = False):
    """numpy in, numpy out: (y,) or, with ``gy`` (or gy=True for its shape only), (y, g_ex, g_log_mag) of sum(y * gy)."""
    x = torch.tensor(np.asarray(ex, dtype=np.float64), requires_grad=gy is not None)
    lm = torch.tensor(np.asarray(log_mag, dtype=np.float64), requires_grad=gy is not None)
    h = min_phase_kernels(lm, torch.as_tensor(np.asarray(window, dtype=np.float64)))
    y = (causal_samplewise if samplewise else causal_frames)(x, h, hop)
    if gy is None:
        return y.detach().numpy()
    (y * torch.as_tensor(np.asarray(gy, dtype=np.float64))).sum().backward()
    return y.detach().numpy(), x.grad.numpy(), lm.grad.numpy()
