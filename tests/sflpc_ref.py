"""Float64 restatement of the source-compensated LPC analysis (golf_lpc_source_filter_f32, include/golf_amd.h; TEST
INFRASTRUCTURE, torch, on whatever device the input lives): iterative adaptive inverse filtering without the integrators,
run on the lags of the windowed frame.  Frames, window, regularisation and ``levinson`` are those of
tests/lpc_analysis_ref.py.

    r[j] = sum_{n < W-j} s[n] s[n+j], j = 0..J = M + Q;   r[0] <- r[0] (1 + eps_rel) + eps_abs
    lags of the frame filtered by c (order P, c_0 = 1):
        rho[d] = sum_{p=0}^{P-d} c_p c_{p+d};   (r o c)[j] = rho[0] r[j] + sum_{d=1}^{P} rho[d] (r[|j-d|] + r[j+d])
    g = lev_1(r) (adaptive) or (-preemphasis);  I times: vt = lev_M((r o g)[0..M]), g = lev_Q((r o vt)[0..Q])
    (a, rc) = lev_M((r o g)[0..M]);   gain = sqrt(max((r o a)[0], 0) / sum(window**2));   source = g_1..g_Q, zero padded

Also here: the planted construction of tools/glottal_preemphasis.py (pulses of the package's table at a constant table
position through a fixed 5-formant all-pole filter) and the chain that scores an analysis on it, shared by
tests/test_sflpc_host.py and tests/test_gpu_sflpc.py."""
import numpy as np
import torch

import lpc_analysis_ref as L

FORMANTS = ((700.0, 90.0), (1220.0, 110.0), (2600.0, 160.0), (3500.0, 200.0), (4500.0, 250.0))   # Hz, bandwidth
HOP, WINDOW, ORDER = 240, 960, 22   # the planted case's analysis: periodic Hann, centred


def poly(a: torch.Tensor) -> torch.Tensor:
    """a_1..a_P (..., P) -> c_0..c_P with c_0 = 1."""
    return torch.cat([torch.ones_like(a[..., :1]), a], -1)


def poly_lags(c: torch.Tensor) -> torch.Tensor:
    """rho[d] = sum_{p=0}^{P-d} c_p c_{p+d}, ascending p."""
    P = c.shape[-1] - 1
    rho = []
    for d in range(P + 1):
        acc = c[..., 0] * c[..., d]
        for p in range(1, P - d + 1):
            acc = acc + c[..., p] * c[..., p + d]
        rho.append(acc)
    return torch.stack(rho, -1)


def filtered_lags(r: torch.Tensor, c: torch.Tensor, n: int) -> torch.Tensor:
    """(r o c)[0..n] from r (..., >= n + P + 1) and c (..., P + 1), ascending d."""
    P = c.shape[-1] - 1
    assert r.shape[-1] >= n + P + 1
    rho = poly_lags(c)
    out = []
    for j in range(n + 1):
        acc = rho[..., 0] * r[..., j]
        for d in range(1, P + 1):
            acc = acc + rho[..., d] * (r[..., abs(j - d)] + r[..., j + d])
        out.append(acc)
    return torch.stack(out, -1)


def frame_lags(x, window, hop: int, J: int, centred: bool = True, n_frames: int = None, eps_rel: float = 1e-9,
               eps_abs: float = 1e-12) -> torch.Tensor:
    """x (B, T), window (W,) -> the regularised lags r (B, F, J + 1) in float64."""
    x = torch.as_tensor(np.array(x) if isinstance(x, np.ndarray) else x).double()   # (a read-only array is copied)
    window = torch.as_tensor(window).double().to(x.device)
    W = window.numel()
    s = L.frames(x, W, hop, centred, n_frames) * window
    r = [(s[..., : W - j] * s[..., j:]).sum(-1) for j in range(J + 1)]
    r[0] = r[0] * (1.0 + eps_rel) + eps_abs
    return torch.stack(r, -1)


def from_lags(r: torch.Tensor, window_energy, M: int, Q: int = 4, iterations: int = 2, preemphasis: float = None):
    """Steps 4 to 7 of the definition on r (..., M + Q + 1) -> (gain, a, rc, source)."""
    if preemphasis is None:
        g = L.levinson(r, 1)[0]
    else:
        g = torch.full_like(r[..., :1], -float(preemphasis))
    for _ in range(iterations):
        vt = L.levinson(filtered_lags(r, poly(g), M), M)[0]
        g = L.levinson(filtered_lags(r, poly(vt), Q), Q)[0]
    a, rc, _ = L.levinson(filtered_lags(r, poly(g), M), M)
    err = filtered_lags(r, poly(a), 0)[..., 0]
    gain = torch.sqrt(torch.clamp(err, min=0.0) / window_energy)
    source = torch.nn.functional.pad(g, (0, Q - g.shape[-1]))
    return gain, a, rc, source


def analysis(x, window, hop: int, M: int, Q: int = 4, iterations: int = 2, preemphasis: float = None, centred: bool = True,
             n_frames: int = None, eps_rel: float = 1e-9, eps_abs: float = 1e-12):
    """x (B, T), window (W,) -> (gain (B, F), a (B, F, M), rc (B, F, M), source (B, F, Q)) in float64."""
    r = frame_lags(x, window, hop, M + Q, centred, n_frames, eps_rel, eps_abs)
    w = torch.as_tensor(window).double().to(r.device)
    return from_lags(r, (w * w).sum(), M, Q, iterations, preemphasis)


# ---- the planted construction ------------------------------------------------------------------------------------------------
def allpole() -> np.ndarray:
    """The denominator 1, a_1 .. a_10 of the five formants at the planted case's sample rate."""
    import glottal_ref as G

    a = np.ones(1)
    for fc, bw in FORMANTS:
        rad = np.exp(-np.pi * bw / G.SR)
        a = np.convolve(a, [1.0, -2 * rad * np.cos(2 * np.pi * fc / G.SR), rad * rad])
    return a


def synth(e: np.ndarray, a: np.ndarray) -> np.ndarray:
    """y[t] = e[t] - sum_{i >= 1} a_i y[t-i], from rest."""
    n = len(a) - 1
    y = np.zeros(len(e) + n)
    ar = a[:0:-1]
    for t in range(len(e)):
        y[t + n] = e[t] - ar @ y[t:t + n]
    return y[n:]


_cache = {}


def planted(w0: float) -> dict:
    """The planted case at the constant table position ``w0``: ``case`` (glottal_ref.build_case: pulses of the package's
    table on the planted f0 track, 1 % noise; its x is the excitation), ``e`` the excitation in float64 and ``y`` the audio,
    both (T,), T = 39 * 240 + 1: 40 frames of one row."""
    import glottal_ref as G

    if w0 not in _cache:
        f0, _ = G.planted_tracks()
        case = G.build_case(G.golf_table(), 64, 256, list(f0), [np.full(f0.shape[1], w0)], 31, noise=0.01)
        e = case["x"][0].astype(np.float64)
        y = synth(e, allpole())
        for arr in (e, y):
            arr.setflags(write=False)
        _cache[w0] = dict(case=case, e=e, y=y)
    return _cache[w0]


def preemphasised(y: np.ndarray, c: float = 0.97) -> np.ndarray:
    return np.concatenate([[y[0]], y[1:] - c * y[:-1]])


def rms(v) -> float:
    v = np.asarray(v, np.float64)
    return float(np.sqrt(np.mean(v * v)))


def worth(pl: dict, e_hat: np.ndarray):
    """An excitation estimate (1, T) of a planted case -> (largest, rms) error of w in table steps on interior frames, by the
    float64 harmonic analysis and match of tests/glottal_ref.py."""
    import glottal_ref as G

    case = pl["case"]
    amp, ph = G.harmonics(case, np.asarray(e_hat, np.float32))
    w_max, w_rms, _ = G.planted_errors(case, G.run(case, amp, ph))
    return w_max, w_rms


def planted_score(pl: dict, gain, a):
    """(gain (1, F), a (1, F, M)) of an analysis of a planted case -> (w max, w rms, rms of the residual of the audio)."""
    import residual_ref

    e_hat = residual_ref.residual(pl["y"][None], np.asarray(gain, np.float64), np.asarray(a, np.float64), HOP)
    return (*worth(pl, e_hat), rms(e_hat))
