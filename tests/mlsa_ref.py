"""The mel-cepstral response of include/golf_amd.h in numpy float64, forward and backward (test infrastructure).

    theta_k = w_k + 2 atan2(alpha sin w_k, 1 - alpha cos w_k),   w_k = 2 pi k / N,   k = 0 .. N/2
    L_k = sum_m mc[m] (cos(m theta_k) - j sin(m theta_k)),   H_k = exp(L_k)
    g_mc[m] = sum_k (P_k cos(m theta_k) + Q_k sin(m theta_k)),   P + jQ = conj(g_h_k) H_k     (g_h = d/d re + j d/d im)
"""
import numpy as np


def theta(n_fft: int, alpha: float) -> np.ndarray:
    w = 2.0 * np.pi * np.arange(n_fft // 2 + 1, dtype=np.float64) / n_fft
    return w + 2.0 * np.arctan2(alpha * np.sin(w), 1.0 - alpha * np.cos(w))


def tables(n_fft: int, order: int, alpha: float):
    """cos(m theta_k), sin(m theta_k) as (order + 1, n_fft/2 + 1) float64; the sine exactly 0 at bins 0 and n_fft/2."""
    angle = np.arange(order + 1, dtype=np.float64)[:, None] * theta(n_fft, alpha)[None, :]
    c, s = np.cos(angle), np.sin(angle)
    s[:, 0] = s[:, -1] = 0.0
    return c, s


def log_response(mc: np.ndarray, n_fft: int, alpha: float) -> np.ndarray:
    c, s = tables(n_fft, mc.shape[-1] - 1, alpha)
    mc = np.asarray(mc, dtype=np.float64)
    return mc @ c - 1j * (mc @ s)


def response(mc: np.ndarray, n_fft: int, alpha: float) -> np.ndarray:
    return np.exp(log_response(mc, n_fft, alpha))


def response_bwd(g_h: np.ndarray, mc: np.ndarray, n_fft: int, alpha: float) -> np.ndarray:
    c, s = tables(n_fft, mc.shape[-1] - 1, alpha)
    pq = np.conj(np.asarray(g_h, dtype=np.complex128)) * response(mc, n_fft, alpha)
    return pq.real @ c.T + pq.imag @ s.T
