"""Plain float64 numpy references of the packed-FIR family (csrc/noise_fir.hip) and of the oscillator's decimator
(csrc/glottal_osc.hip), written from the definitions in the kernels' header comments with loops over the taps, plus
the cases and inputs shared by tests/test_fir_ref_host.py (CPU) and tests/test_gpu_fir_family.py (GPU).

  LTI FIR      y[b,t]       = sum_n taps[n] ex[b, t-lead+n], zero outside [0,T)
  frame FIR    y[b,f*hop+n] = sum_k kern[b,f+frame0,k] pad(ex)[b,f*hop+n+k]         (zero-phase, P = (N-1)//2 each side)
               y[b,f*hop+n] = sum_j kern[b,f+frame0,j] ex[b,f*hop+n-j]              (causal)
  decimator    out[b,o]     = sum_k taps[k] x[b, o*os+k-half], half = (K-1)//2, Tout = (N-1)//os + 1
"""
import numpy as np

FWD_BAR, GRAD_BAR = 1e-5, 2e-5     # the project's own bars (tests/test_gpu_noise_fir.py): forward, gradients


# ------------------------------------------------------------------------------------------------ LTI FIR
def _shifted(x, s):
    """z[:, t] = x[:, t + s], zero outside [0, T)."""
    T = x.shape[1]
    z = np.zeros_like(x)
    lo, hi = max(0, -s), min(T, T - s)
    if hi > lo:
        z[:, lo:hi] = x[:, lo + s: hi + s]
    return z


def lti_fir(ex, taps, lead):
    ex, taps = np.asarray(ex, np.float64), np.asarray(taps, np.float64)
    y = np.zeros_like(ex)
    for n in range(taps.shape[0]):
        y += taps[n] * _shifted(ex, n - lead)
    return y


def lti_fir_grads(gy, ex, taps, lead):
    gy, ex, taps = (np.asarray(v, np.float64) for v in (gy, ex, taps))
    g_ex = np.zeros_like(ex)
    g_taps = np.zeros_like(taps)
    for n in range(taps.shape[0]):
        g_taps[n] = (gy * _shifted(ex, n - lead)).sum()
        g_ex += taps[n] * _shifted(gy, lead - n)      # ex[u] reaches y[u + lead - n]
    return g_ex, g_taps


# ------------------------------------------------------------------------------------------------ frame FIR
def frames_count(T, F, N, hop, causal, frame0=0):
    pad = N - 1 if causal else 2 * ((N - 1) // 2)
    assert T + pad >= N + hop - 1, "shorter than one frame span"
    return min((T + pad - (N + hop - 1)) // hop + 1, F - frame0)


def frames_min_length(N, hop, causal):
    """Smallest legal excitation: exactly one frame."""
    pad = N - 1 if causal else 2 * ((N - 1) // 2)
    return max(1, N + hop - 1 - pad)


def _frames_pad(ex, N, causal):
    """xp with xp[:, m] = ex[:, m - P] and enough zeros behind; kernel index k reads xp[f*hop+n+k] (causal: k = N-1-j)."""
    P = N - 1 if causal else (N - 1) // 2
    return P, np.pad(ex, ((0, 0), (P, N)))


def frames_fir(ex, kern, hop, causal, frame0=0):
    ex, kern = np.asarray(ex, np.float64), np.asarray(kern, np.float64)
    B, T = ex.shape
    _, F, N = kern.shape
    nfr = frames_count(T, F, N, hop, causal, frame0)
    P, xp = _frames_pad(ex, N, causal)
    y = np.zeros((B, nfr * hop))
    for f in range(nfr):
        row = kern[:, f + frame0]
        for k in range(N):
            c = row[:, N - 1 - k] if causal else row[:, k]
            y[:, f * hop: (f + 1) * hop] += c[:, None] * xp[:, f * hop + k: f * hop + k + hop]
    return y


def frames_fir_grads(gy, ex, kern, hop, causal, frame0=0):
    gy, ex, kern = (np.asarray(v, np.float64) for v in (gy, ex, kern))
    B, T = ex.shape
    _, F, N = kern.shape
    nfr = frames_count(T, F, N, hop, causal, frame0)
    assert gy.shape == (B, nfr * hop)
    P, xp = _frames_pad(ex, N, causal)
    g_xp = np.zeros_like(xp)
    g_kern = np.zeros_like(kern)
    for f in range(nfr):
        g = gy[:, f * hop: (f + 1) * hop]
        row = kern[:, f + frame0]
        for k in range(N):
            j = N - 1 - k if causal else k
            g_kern[:, f + frame0, j] = (g * xp[:, f * hop + k: f * hop + k + hop]).sum(-1)
            g_xp[:, f * hop + k: f * hop + k + hop] += row[:, j, None] * g
    return g_xp[:, P: P + T], g_kern


# ------------------------------------------------------------------------------------------------ decimator
def _decim_hits(k, half, os, N, Tout):
    """Outputs o whose tap k falls inside the signal, and the sample m = o*os + k - half it reads."""
    o = np.arange(Tout)
    m = o * os + k - half
    ok = (m >= 0) & (m < N)
    return o[ok], m[ok]


def decimate(x, taps, os):
    x, taps = np.asarray(x, np.float64), np.asarray(taps, np.float64)
    B, N = x.shape
    K = taps.shape[0]
    half, Tout = (K - 1) // 2, (N - 1) // os + 1
    out = np.zeros((B, Tout))
    for k in range(K):
        o, m = _decim_hits(k, half, os, N, Tout)
        out[:, o] += taps[k] * x[:, m]
    return out


def decimate_adjoint(g, taps, os, N):
    g, taps = np.asarray(g, np.float64), np.asarray(taps, np.float64)
    B, Tout = g.shape
    K = taps.shape[0]
    half = (K - 1) // 2
    assert Tout == (N - 1) // os + 1
    gx = np.zeros((B, N))
    for k in range(K):
        o, m = _decim_hits(k, half, os, N, Tout)
        gx[:, m] += taps[k] * g[:, o]      # m is distinct for distinct o: no repeated index
    return gx


# ------------------------------------------------------------------------------------------------ float32 emulation
def seq32(terms):
    """Sequential float32 sum along the last axis of float32-rounded products: what one fp32 accumulator does (an FMA chain
    is no worse)."""
    t = np.asarray(terms, np.float64).astype(np.float32)
    if t.shape[-1] == 0:
        return np.zeros(t.shape[:-1], np.float32)
    return np.cumsum(t, axis=-1, dtype=np.float32)[..., -1]


def _win(xp, width):
    return np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)


def lti_fir_f32(ex, taps, lead):
    ex32 = np.asarray(ex, np.float32).astype(np.float64)
    t32 = np.asarray(taps, np.float32).astype(np.float64)
    K, T = t32.shape[0], ex32.shape[1]
    xp = np.pad(ex32, ((0, 0), (lead, K - 1 - lead)))
    return seq32(_win(xp, K)[:, :T] * t32)


def lti_fir_grads_f32(gy, ex, taps, lead):
    gy32 = np.asarray(gy, np.float32).astype(np.float64)
    ex32 = np.asarray(ex, np.float32).astype(np.float64)
    K = np.asarray(taps).shape[0]
    g_ex = lti_fir_f32(gy, np.asarray(taps)[::-1], K - 1 - lead)
    B, T = ex32.shape
    xp = np.pad(ex32, ((0, 0), (lead, K - 1 - lead)))
    g_taps = np.stack([seq32((gy32 * xp[:, n: n + T]).reshape(-1)) for n in range(K)])
    return g_ex, g_taps


def frames_fir_f32(ex, kern, hop, causal, frame0=0):
    ex32 = np.asarray(ex, np.float32).astype(np.float64)
    k32 = np.asarray(kern, np.float32).astype(np.float64)
    B, T = ex32.shape
    _, F, N = k32.shape
    nfr = frames_count(T, F, N, hop, causal, frame0)
    _, xp = _frames_pad(ex32, N, causal)
    y = np.zeros((B, nfr * hop), np.float32)
    for f in range(nfr):
        row = k32[:, f + frame0, ::-1] if causal else k32[:, f + frame0]
        w = _win(xp[:, f * hop: f * hop + hop + N - 1], N)           # (B, hop, N)
        y[:, f * hop: (f + 1) * hop] = seq32(w * row[:, None, :])
    return y


def frames_fir_grads_f32(gy, ex, kern, hop, causal, frame0=0):
    gy32 = np.asarray(gy, np.float32).astype(np.float64)
    ex32 = np.asarray(ex, np.float32).astype(np.float64)
    k32 = np.asarray(kern, np.float32).astype(np.float64)
    B, T = ex32.shape
    _, F, N = k32.shape
    nfr = frames_count(T, F, N, hop, causal, frame0)
    P, xp = _frames_pad(ex32, N, causal)
    g_kern = np.zeros(k32.shape, np.float32)
    # g_xp[m] = sum_f sum_n gy[f*hop+n] row_f[m - f*hop - n]: one accumulator per sample, frames and n in ascending order
    contrib = [[] for _ in range(xp.shape[1])]
    for f in range(nfr):
        g = gy32[:, f * hop: (f + 1) * hop]
        w = _win(xp[:, f * hop: f * hop + hop + N - 1], hop)         # (B, N, hop): w[:, k, n] = xp[f*hop+n+k]
        gk = seq32(w * g[:, None, :])
        g_kern[:, f + frame0] = gk[:, ::-1] if causal else gk
        row = k32[:, f + frame0, ::-1] if causal else k32[:, f + frame0]
        for n in range(hop):
            for k in range(N):
                contrib[f * hop + n + k].append(g[:, n] * row[:, k])
    g_xp = np.zeros(xp.shape, np.float32)
    for m, c in enumerate(contrib):
        if c:
            g_xp[:, m] = seq32(np.stack(c, -1))
    return g_xp[:, P: P + T], g_kern


def decimate_f32(x, taps, os):
    x32 = np.asarray(x, np.float32).astype(np.float64)
    t32 = np.asarray(taps, np.float32).astype(np.float64)
    B, N = x32.shape
    K = t32.shape[0]
    half, Tout = (K - 1) // 2, (N - 1) // os + 1
    xp = np.pad(x32, ((0, 0), (half, half + os)))
    return seq32(_win(xp, K)[:, : (Tout - 1) * os + 1: os] * t32)


def decimate_adjoint_f32(g, taps, os, N):
    g32 = np.asarray(g, np.float32).astype(np.float64)
    t32 = np.asarray(taps, np.float32).astype(np.float64)
    B, Tout = g32.shape
    K = t32.shape[0]
    half = (K - 1) // 2
    gx = np.zeros((B, N), np.float32)
    for m in range(N):
        o = np.arange(max(0, -(-(m + half - K + 1) // os)), min(Tout - 1, (m + half) // os) + 1)
        gx[:, m] = seq32(g32[:, o] * t32[m - o * os + half])
    return gx


# ------------------------------------------------------------------------------------------------ the shared cases
# (B, T, ntaps, lead): what each one exercises is in the GPU test's table
LTI_CASES = [(3, 253, 4, 0), (3, 253, 4, 3), (2, 1, 8, 0), (1, 3, 12, 11), (2, 252, 8, 5), (2, 961, 252, 100),
             (2, 962, 252, 0), (2, 1923, 264, 0), (2, 1923, 264, 101), (2, 1923, 264, 263), (2, 2883, 512, 200)]
LTI_LARGEST = (1, 300, 3836, 1000)
LTI_BATCH = (5, 700, 264, 101)     # 5 rows x 3 tiles = 15 units: not a multiple of the 4 waves of a workgroup


def lti_inputs(B, T, ntaps, lead):
    rng = np.random.default_rng([B, T, ntaps, lead])
    f32 = lambda v: v.astype(np.float32)   # noqa: E731 -- the values the GPU sees, exactly
    return f32(rng.normal(0, 1, (B, T))), f32(rng.normal(0, 1, ntaps)), f32(rng.normal(0, 1, (B, T)))


def _frames_case(N, hop, F, B=2, T=None, frame0=0):
    return dict(N=N, hop=hop, F=F, B=B, T=T, frame0=frame0)


# T = None: F*hop + min(40, hop-1): every kernel row is used in both alignments and the causal wrapper's T // hop <= F holds;
# "min": the smallest legal length
FRAMES_CASES = {}
for _N in (5, 7):
    for _hop in (4, 48):
        FRAMES_CASES[f"small-N{_N}-hop{_hop}"] = _frames_case(_N, _hop, 4)
for _N in (48, 49, 50, 51):
    FRAMES_CASES[f"mod4-N{_N}"] = _frames_case(_N, 24, 5)
for _N in (251, 252, 253, 505):
    FRAMES_CASES[f"pass-N{_N}"] = _frames_case(_N, 120, 3)
for _hop in (248, 252, 256, 504, 508):
    FRAMES_CASES[f"tile-hop{_hop}"] = _frames_case(30, _hop, 3)
FRAMES_CASES["many-frames"] = _frames_case(51, 4, 40)
FRAMES_CASES["one-frame"] = _frames_case(21, 24, 2, T="min")
FRAMES_CASES["long-tail"] = _frames_case(21, 24, 3, T=3 * 24 + 700)       # T far past the last frame's reach
FRAMES_CASES["unused-rows"] = _frames_case(30, 48, 7, T=4 * 48 + 35)      # nfr = 4, F = nfr + 3
for _f0 in (0, 1, 2):
    FRAMES_CASES[f"frame0-{_f0}"] = _frames_case(22, 40, 6, frame0=_f0, T=3 * 40 + 25)   # nfr = 3 of F = 6 rows
FRAMES_ODD_HOPS = (1, 3, 7, 250)          # forward only: the backward refuses them
for _hop in FRAMES_ODD_HOPS:
    FRAMES_CASES[f"odd-hop{_hop}"] = _frames_case(30, _hop, 5)
FRAMES_CASES["largest-N"] = _frames_case(3836, 8, 2, B=1, T=300)
FRAMES_CASES["largest-hop"] = _frames_case(8, 3836, 1, B=1, T=3836 + 300)


def frames_inputs(cid, causal):
    """-> the case plus T, nfr, ex (B,T), kern (B,F,N) scaled by 1/N, gy (B, nfr*hop): float32 values, asymmetric kernels."""
    c = dict(FRAMES_CASES[cid])
    N, hop, F, B, frame0 = c["N"], c["hop"], c["F"], c["B"], c["frame0"]
    if c["T"] == "min":
        T = frames_min_length(N, hop, causal)
    elif c["T"] is None:
        T = F * hop + min(40, hop - 1)
    else:
        T = c["T"]
    nfr = frames_count(T, F, N, hop, causal, frame0)
    rng = np.random.default_rng([N, hop, F, B, frame0, int(causal), sum(map(ord, cid))])
    f32 = lambda v: v.astype(np.float32)   # noqa: E731
    c.update(T=T, nfr=nfr, causal=causal, ex=f32(rng.normal(0, 1, (B, T))), kern=f32(rng.normal(0, 1, (B, F, N)) / N),
             gy=f32(rng.normal(0, 1, (B, nfr * hop))))
    return c


def frames_reach(c):
    """One past the last excitation sample any used frame reads."""
    N, hop, nfr = c["N"], c["hop"], c["nfr"]
    P = N - 1 if c["causal"] else (N - 1) // 2
    return min(c["T"], nfr * hop + (0 if c["causal"] else N - 1 - P))


def decimator_taps(os):
    from golf_amd.synth import Decimate

    return Decimate(os).taps.numpy().copy()


def decim_lengths(os):
    """N with Tout in {1, 2, 1024, 1025}, and N in {1, os, os+1}."""
    return sorted({1, os, os + 1, (1024 - 1) * os + 1, 1024 * os, 1024 * os + 1})


# (os, K or None for the designed taps, N)
DECIM_CASES = [(os, None, N) for os in (2, 3, 4) for N in decim_lengths(os)]
DECIM_CASES += [(os, K, N) for os in (5, 8) for K in (1, 3, 31, 255) for N in (os + 1, 1024 * os + 1)]
DECIM_CASES += [(5, 31, N) for N in decim_lengths(5) if N not in (6, 5121)]
DECIM_ADJ_CASES = [(2, None, 2049), (3, None, 3073), (5, 31, 5121), (5, 255, 777), (4, None, 4097), (4, None, 12000),
                   (2, None, 1), (3, None, 4), (4, None, 5)]
DECIM_FILL = (4, None, 12000)


def decim_inputs(os, K, N, B=2):
    rng = np.random.default_rng([os, K or 0, N, B])
    f32 = lambda v: v.astype(np.float32)   # noqa: E731
    x = f32(rng.normal(0, 1, (B, N)))
    taps = decimator_taps(os) if K is None else f32(rng.normal(0, 1, K))
    g = f32(rng.normal(0, 1, (B, (N - 1) // os + 1)))
    return x, taps, g
