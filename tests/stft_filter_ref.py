"""Float64 restatement of the STFT-domain frame filter and of its backward (TEST INFRASTRUCTURE; numpy on the CPU).

Forward, as include/golf_amd.h states it, with n = n_fft, w = window, pad = n/2:

    frames = min(1 + T // hop, F),  Ty = hop * (frames - 1)
    v_f[k] = w[k] x[refl(f*hop - pad + k)],  refl(i) = -i for i < 0 and 2(T-1) - i for i >= T
    V_f = FFT(v_f),  u_f = Re IFFT(V_f Hext_f),  Hext the Hermitian extension of the rows given on bins 0 .. n/2
    y[m] = sum_f w[k] u_f[k] / norm[m],  norm[m] = sum_f w[k]^2,  k = m + pad - f*hop,  m in [0, Ty)

Backward for gy (B, Ty), the closed form golf_stft_filter_frames_bwd_f32 evaluates:

    q = gy / norm,  gu_f[k] = w[k] q[f*hop - pad + k] (0 outside [0, Ty)),  GU_f = FFT(gu_f)
    gH_f[kk] = c[kk] conj(V_f[kk]) GU_f[kk] / n on bins 0 .. n/2, c = 1 at 0 and n/2, 2 elsewhere (real rows: its real part);
               rows frames <= f < F are zero
    gv_f = Re IFFT(conj(Hext_f) GU_f),  G[p] = sum_f w[k] gv_f[k] on the padded positions p in [-pad, (frames-1)*hop + pad)
    gx[r] = G[r] + G[-r] (1 <= r <= pad) + G[2(T-1) - r] (where that position is >= T and inside the padded range)

tests/test_stft_filter_grad_host.py pins both to float64 autograd through LTVCepFilter / DiffWorldSPFilter at 1e-12."""
import numpy as np


def _frames(x, H, w, hop):
    """(frames, Ty, V (B, frames, n), Hext (B, frames, n), norm (L,)) with L = (frames-1)*hop + n padded positions."""
    T, F, n = x.shape[1], H.shape[1], w.shape[0]
    pad = n // 2
    assert H.shape[2] == pad + 1 and T > pad and n >= 2 * hop
    frames = min(1 + T // hop, F)
    idx = np.arange(frames)[:, None] * hop - pad + np.arange(n)[None, :]
    idx = np.where(idx < 0, -idx, idx)
    idx = np.where(idx >= T, 2 * (T - 1) - idx, idx)
    V = np.fft.fft(w * x[:, idx], axis=-1)
    Hh = H[:, :frames].astype(np.complex128)
    Hext = np.concatenate([Hh, np.conj(Hh[..., -2:0:-1])], axis=-1)
    norm = np.zeros((frames - 1) * hop + n)
    for f in range(frames):
        norm[f * hop: f * hop + n] += w * w
    return frames, hop * (frames - 1), V, Hext, norm


def _overlap_add(w, u, hop):
    B, frames, n = u.shape
    out = np.zeros((B, (frames - 1) * hop + n))
    for f in range(frames):
        out[:, f * hop: f * hop + n] += w * u[:, f]
    return out


def forward(x, H, w, hop):
    """x (B, T), H (B, F, n/2+1) real or complex, w (n,) -> y (B, Ty)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    pad = w.shape[0] // 2
    frames, Ty, V, Hext, norm = _frames(x, H, w, hop)
    u = np.fft.ifft(V * Hext, axis=-1).real
    return _overlap_add(w, u, hop)[:, pad: pad + Ty] / norm[pad: pad + Ty]


def backward(gy, x, H, w, hop):
    """-> (gx (B, T), gH like H: complex (d/d re + i d/d im, torch's convention) for complex rows, real for real rows)."""
    gy, x, w = np.asarray(gy, np.float64), np.asarray(x, np.float64), np.asarray(w, np.float64)
    H = np.asarray(H)
    (B, T), n = x.shape, w.shape[0]
    pad = n // 2
    frames, Ty, V, Hext, norm = _frames(x, H, w, hop)
    assert gy.shape == (B, Ty)
    L = (frames - 1) * hop + n
    q = np.zeros((B, L))
    q[:, pad: pad + Ty] = gy / norm[pad: pad + Ty]
    pos = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]      # padded position + pad
    GU = np.fft.fft(w * q[:, pos], axis=-1)
    c = np.full(pad + 1, 2.0)
    c[0] = c[pad] = 1.0
    gH = np.zeros(H.shape, np.complex128)
    gH[:, :frames] = c * np.conj(V[..., : pad + 1]) * GU[..., : pad + 1] / n
    if not np.iscomplexobj(H):
        gH = gH.real
    gv = np.fft.ifft(np.conj(Hext) * GU, axis=-1).real
    Gp = _overlap_add(w, gv, hop)                                        # Gp[:, p + pad] = G[p]
    G = lambda p: np.where((p + pad >= 0) & (p + pad < L), Gp[:, np.clip(p + pad, 0, L - 1)], 0.0)
    r = np.arange(T)
    gx = G(r) + np.where((r >= 1) & (r <= pad), G(-r), 0.0) + np.where(2 * (T - 1) - r >= T, G(2 * (T - 1) - r), 0.0)
    return gx, gH
