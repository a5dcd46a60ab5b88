"""The fused residual (golf_ltv_residual_f32, include/golf_amd.h) restated in float64, indexed by utterance positions as the
block-by-block entry (golf_ltv_residual_stream_f32) defines them, plus an fp32 stand-in: the same steps in numpy float32
(unfused multiply-adds), whose error against float64 on a case is the scale of that case's parity bar.

x (B, T), gain (B, F) and a (B, F, M) are laid out from position 0 (what a caller does not know may be NaN: a sample or a
frame that the definition does not read never reaches a result).  Sample t:
  f = min(t // hop, F - 2), 0 when F == 1 (``last``: the utterance has the F frames given); t // hop without ``last``
  w = (t - f hop) / hop;  A[i] = a[f, i] + w (a[f+1, i] - a[f, i]);  G = gain[f] + w (gain[f+1] - gain[f])
  e[t] = (x[t] + sum_{i < M, t-1-i >= 0} A[i] x[t-1-i]) / G, the sum in ascending i.
Every step is elementwise over the samples, so a sample's value does not depend on which other samples are computed with it.
"""
import numpy as np


def length(T, F, hop):
    """T' = min(T, (F - 1) hop + 1), 0 without a frame."""
    return min(T, (F - 1) * hop + 1) if F >= 1 else 0


def residual(x, gain, a, hop, t_first=0, n_out=None, last=True, fp32=False):
    """Samples ``t_first .. t_first + n_out - 1`` (to the end of the utterance when ``n_out`` is None), (B, n_out)."""
    x, gain, a = np.asarray(x), np.asarray(gain), np.asarray(a)
    assert x.ndim == 2 and gain.ndim == 2 and a.ndim == 3 and a.shape[:2] == gain.shape and x.shape[0] == gain.shape[0]
    dt = np.float32 if fp32 else np.float64
    (B, T), (F, M) = x.shape, a.shape[1:]
    if n_out is None:
        assert last
        n_out = length(T, F, hop) - t_first
    t = np.arange(t_first, t_first + n_out)
    assert n_out >= 0 and (n_out == 0 or t[-1] < T)
    if last:
        assert n_out == 0 or t[-1] < (F - 1) * hop + 1
        f = np.minimum(t // hop, F - 2) if F >= 2 else np.zeros_like(t)
        f1 = f + 1 if F >= 2 else f
    else:
        f, f1 = t // hop, t // hop + 1
        assert n_out == 0 or f1[-1] < F
    w = (t - f * hop).astype(dt) / dt(hop)
    out = np.empty((B, n_out), dt)
    with np.errstate(all="ignore"):
        for b in range(B):
            a0, a1, g0, g1 = a[b, f].astype(dt), a[b, f1].astype(dt), gain[b, f].astype(dt), gain[b, f1].astype(dt)
            A = a0 + w[:, None] * (a1 - a0)
            G = g0 + w * (g1 - g0)
            xb = x[b].astype(dt)
            acc = xb[t]
            for i in range(M):
                idx = t - 1 - i
                acc = np.where(idx >= 0, acc + A[:, i] * xb[np.maximum(idx, 0)], acc)
            out[b] = acc / G
    return out


def error(got, ref):
    """The largest error in units of the case's largest reference magnitude."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max(initial=0.0) / max(np.abs(ref).max(initial=0.0), 1e-300))


def inputs(B, F, M, T, seed):
    """fp32 inputs in the style of tests/test_gpu_lpc_inverse.py, with gains of either side of 1."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (B, T)).astype(np.float32)
    a = (rng.normal(0, 1, (B, F, M)) * 0.5 / np.sqrt(M)).astype(np.float32)
    gain = np.exp(rng.uniform(-1.5, 1.5, (B, F))).astype(np.float32)
    return x, gain, a
