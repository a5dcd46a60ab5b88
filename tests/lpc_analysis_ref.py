"""Float64 restatement of the frame-wise LPC analysis (TEST INFRASTRUCTURE; torch, autograd for the gradients).

The definition of include/golf_amd.h written out as it stands, on whatever device the input lives:

    frame f, tap k reads x[f*hop - W//2 + k] (centred, F = T // hop + 1) or x[f*hop + k] (F = max(T - W, 0) // hop + 1),
    zeros outside [0, T); n_frames overrides F
    s = frame * window;   r[j] = sum_{n < W-j} s[n] s[n+j], j = 0..M;   r[0] <- r[0] (1 + eps_rel) + eps_abs
    Levinson-Durbin as levinson() of oracle/make_lpc_tracks.py
    a (B, F, M),  rc (B, F, M) = k_1..k_M,  gain (B, F) = sqrt(max(E_M, 0) / sum(window**2))

tests/test_lpc_analysis_host.py pins it to oracle.make_lpc_tracks.analyse at 1e-9."""
import numpy as np
import torch


def n_frames_of(T: int, W: int, hop: int, centred: bool = True) -> int:
    return T // hop + 1 if centred else max(T - W, 0) // hop + 1


def frames(x: torch.Tensor, W: int, hop: int, centred: bool = True, n_frames: int = None) -> torch.Tensor:
    """x (B, T) -> (B, F, W), zeros outside the signal."""
    B, T = x.shape
    F = n_frames_of(T, W, hop, centred) if n_frames is None else n_frames
    left = W // 2 if centred else 0
    right = max((F - 1) * hop + W - left - T, 0)
    xp = torch.nn.functional.pad(x, (left, right))
    return xp.unfold(1, W, hop)[:, :F]


def levinson(r: torch.Tensor, M: int):
    """r (..., M+1) -> a (..., M), rc (..., M), err (...)."""
    a = []                      # a[j-1] = a_j of the current stage
    ks = []
    err = r[..., 0]
    for i in range(1, M + 1):
        acc = r[..., i]
        for j in range(1, i):
            acc = acc + a[j - 1] * r[..., i - j]
        k = -acc / err
        a = [a[j - 1] + k * a[i - j - 1] for j in range(1, i)] + [k]
        ks.append(k)
        err = err * (1.0 - k * k)
    return torch.stack(a, -1), torch.stack(ks, -1), err


def analysis(x, window, hop: int, M: int, centred: bool = True, n_frames: int = None, eps_rel: float = 1e-9,
             eps_abs: float = 1e-12):
    """x (B, T), window (W,) -> (gain, a, rc) in float64; differentiable w.r.t. x."""
    x = torch.as_tensor(x).double()
    window = torch.as_tensor(window).double().to(x.device)
    W = window.numel()
    s = frames(x, W, hop, centred, n_frames) * window
    r = [(s[..., : W - j] * s[..., j:]).sum(-1) for j in range(M + 1)]
    r[0] = r[0] * (1.0 + eps_rel) + eps_abs
    a, rc, err = levinson(torch.stack(r, -1), M)
    gain = torch.sqrt(torch.clamp(err, min=0.0) / (window * window).sum())
    return gain, a, rc


def analysis_with_grads(x, window, hop, M, cot, **kw):
    """cot = (g_gain, g_a, g_rc), each an array or None.  Returns (gain, a, rc, g_x) as numpy float64."""
    xt = torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True)
    out = analysis(xt, window, hop, M, **kw)
    loss = sum((o * torch.as_tensor(np.asarray(g)).double()).sum() for o, g in zip(out, cot) if g is not None)
    (g_x,) = torch.autograd.grad(loss, xt)
    return tuple(o.detach().numpy() for o in out) + (g_x.numpy(),)


def speech_like(golden, rows, T: int, hop: int = 240, seed: int = 0) -> np.ndarray:
    """Seeded N(0,1) noise through the all-pole filters of tests/golden/g25 (speech tracks, order 22, frames [:21]):
    audio with the conditioning of speech (reflection coefficients up to 0.998) without committing any."""
    from oracle import golf_oracle as O

    g = golden("g25_speech_lpc_tracks")
    a = g["a"][list(rows), :21].astype(np.float64)
    gain = g["gain"][list(rows), :21].astype(np.float64)
    ex = np.random.default_rng(seed).normal(0, 1, (len(rows), T))
    return O.ltv_allpole_ss_forward(ex, gain / gain.max(), a, hop)
