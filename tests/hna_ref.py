"""Float64 restatement of the harmonic-plus-noise analysis (golf_harmonic_analysis_f32, include/golf_amd.h), written from the
definition with numpy, one step after the other.  It is the checker of csrc/harm_analysis.hip (tests/test_gpu_hna.py) and is
itself pinned on synthetic signals of known amplitudes by tests/test_hna_host.py.

``fp32=True`` is the stand-in for a plain fp32 kernel: the same steps with the window, the windowed samples, sin and cos,
every product and every sum in float32 (numpy's float32 matrix products), the phase k phi(m) mod 1 still exact.  The host
test holds it to the bars of the GPU test against the float64 version, on the GPU test's own inputs.

Also here: the signals and the cases both test files share."""
import math

import numpy as np

SR, HOP = 24000.0, 240


def window_length(fd, sample_rate, periods, min_window, max_window, unvoiced_window):
    if not fd > 0:
        return unvoiced_window
    n_per = max(periods, math.ceil(min_window * fd / sample_rate))
    return max(2, int(min(max_window, math.floor(n_per * sample_rate / fd + 0.5))))


def chirp(f0row, f, hop, sample_rate):
    """The four rules: central, forward, backward difference of the voiced neighbours' f0, else 0 (cycles per sample^2)."""
    fd = float(f0row[f])
    prev = float(f0row[f - 1]) if f > 0 and f0row[f - 1] > 0 else None
    nxt = float(f0row[f + 1]) if f + 1 < len(f0row) and f0row[f + 1] > 0 else None
    if prev is not None and nxt is not None:
        return (nxt - prev) / (2 * hop * sample_rate), "central"
    if nxt is not None:
        return (nxt - fd) / (hop * sample_rate), "forward"
    if prev is not None:
        return (fd - prev) / (hop * sample_rate), "backward"
    return 0.0, "none"


def analyse(x, f0, sample_rate, hop, K, n_mag=0, periods=4, min_window=None, max_window=2048, unvoiced_window=None,
            smooth=0, eps=1e-12, fp32=False):
    """x (B, T), f0 (B, F) -> dict: amp, phase (B, F, K), log_mag (B, F, n_mag) or None, and per frame L, scale (max |x| over
    the window), voiced, rule (the chirp rule taken)."""
    x, f0 = np.asarray(x), np.asarray(f0)
    assert x.ndim == 2 and f0.ndim == 2 and x.shape[0] == f0.shape[0]
    min_window = 2 * hop if min_window is None else min_window
    unvoiced_window = 4 * hop if unvoiced_window is None else unvoiced_window
    assert periods >= 2 and 1 <= min_window <= max_window and 0 <= smooth and (n_mag == 0 or smooth < n_mag)
    (B, T), F = x.shape, f0.shape[1]
    dt = np.float32 if fp32 else np.float64
    amp, phase = np.zeros((B, F, K)), np.zeros((B, F, K))
    log_mag = np.zeros((B, F, n_mag)) if n_mag else None
    Ls, scale = np.zeros((B, F), int), np.zeros((B, F))
    voiced, rule = np.zeros((B, F), bool), np.empty((B, F), object)
    ks = np.arange(1, K + 1)
    for b in range(B):
        for f in range(F):
            fd = float(f0[b, f])
            v = fd > 0
            L = window_length(fd, sample_rate, periods, min_window, max_window, unvoiced_window)
            # window and offsets
            i = np.arange(L)
            m = -(L // 2) + i
            w = (0.5 - 0.5 * np.cos(2 * np.pi * (i + 0.5) / L)).astype(dt)
            t = f * hop + m
            ok = (t >= 0) & (t < T)
            xs = np.where(ok, x[b, np.clip(t, 0, max(T - 1, 0))] if T else 0.0, 0.0).astype(dt)
            sum_w, sum_w2 = float(w.astype(np.float64).sum()), float((w.astype(np.float64) ** 2).sum())
            Ls[b, f], scale[b, f], voiced[b, f] = L, np.abs(xs).max(), v
            r = xs
            rule[b, f] = "unvoiced"
            if v:
                # phase model
                omega = fd / sample_rate
                s, rule[b, f] = chirp(f0[b], f, hop, sample_rate)
                md = m.astype(np.float64)
                phi = omega * md + s * md * md / 2
                # harmonics
                th = np.outer(ks, phi)
                th -= np.floor(th)
                E = np.exp(-2j * np.pi * th).astype(np.complex64 if fp32 else np.complex128)
                c = (E @ (w * xs).astype(E.dtype)) * dt(2 / sum_w)
                c[ks * omega >= 0.5] = 0
                amp[b, f] = np.abs(c)
                ph = np.angle(c.astype(np.complex128)) / (2 * np.pi) + 0.25
                phase[b, f] = np.where(np.abs(c) > 0, ph - np.floor(ph), 0.25)
                # residual
                r = (xs - (c.conj() @ E).real).astype(dt)   # Re(c_k exp(+2 pi j k phi)) = Re(conj(c_k) E_k)
            if n_mag:
                bins = np.outer(np.arange(n_mag), m.astype(np.float64)) / (2 * (n_mag - 1))
                bins -= np.floor(bins)
                En = np.exp(-2j * np.pi * bins).astype(np.complex64 if fp32 else np.complex128)
                z = En @ (w * r).astype(En.dtype)
                S = (z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2) / sum_w2
                if smooth:
                    pad = np.pad(S, smooth, mode="reflect")
                    S = np.array([pad[j:j + 2 * smooth + 1].mean() for j in range(n_mag)])
                log_mag[b, f] = 0.5 * np.log(S + eps)
    return dict(amp=amp, phase=phase, log_mag=log_mag, L=Ls, scale=scale, voiced=voiced, rule=rule)


def errors(out, ref):
    """The largest errors of ``out`` against ``ref`` in the GPU test's units: amplitude and magnitude in units of the
    frame's scale, phase in units of its allowance scale / amp (cycles, modulo 1, where the reference's amp >= 1e-2 scale)."""
    sc = ref["scale"][..., None]
    live = sc > 0
    safe = np.where(live, sc, 1.0)
    e_amp = (np.abs(out["amp"] - ref["amp"]) / safe)[np.broadcast_to(live, ref["amp"].shape)].max(initial=0.0)
    e_mag = 0.0
    if ref["log_mag"] is not None:
        d = np.abs(np.exp(out["log_mag"]) - np.exp(ref["log_mag"])) / safe
        e_mag = d[np.broadcast_to(live, d.shape)].max(initial=0.0)
    strong = ref["amp"] >= 1e-2 * sc
    strong &= live
    dp = np.abs(out["phase"] - ref["phase"])
    dp = np.minimum(dp, 1 - dp)
    e_ph = (dp * ref["amp"] / safe)[strong].max(initial=0.0)
    return e_amp, e_mag, e_ph


# ---- signals -------------------------------------------------------------------------------------------------------------
def upsample(z, hop):
    """Linear upsampling of the frames z (F, ...) to (F-1)*hop + 1 samples, as the oscillator bank upsamples its controls."""
    F = z.shape[0]
    pos = np.arange((F - 1) * hop + 1) / hop
    lo = np.minimum(pos.astype(int), max(F - 2, 0))
    fr = (pos - lo).reshape((-1,) + (1,) * (z.ndim - 1))
    return z[lo] * (1 - fr) + z[np.minimum(lo + 1, F - 1)] * fr


def bank(f0, amps, hop, sample_rate):
    """The oscillator bank in float64: sum_k up(amps)[:, k] sin(2 pi k cumsum(up(f0) / sr)), harmonics at or above Nyquist
    muted.  f0 (F), amps (F, K) -> (F-1)*hop + 1 samples."""
    p = upsample(np.asarray(f0, np.float64), hop) / sample_rate
    a = upsample(np.asarray(amps, np.float64), hop)
    Phi = np.cumsum(p)
    k = np.arange(1, a.shape[1] + 1)
    return (a * np.sin(2 * np.pi * np.outer(Phi, k)) * (np.outer(p, k) < 0.5)).sum(1)


def track(kind, F, hop=HOP, sample_rate=SR):
    """The f0 tracks of the host test, as fp32 values in Hz per frame."""
    t = np.arange(F) * hop / sample_rate
    f = {"const200": np.full(F, 200.0), "const173": np.full(F, 173.3), "glide150": np.linspace(150.0, 250.0, F),
         "glide80": np.linspace(80.0, 100.0, F),
         "vibrato": 220.0 * 2 ** (0.5 / 12 * np.sin(2 * np.pi * 5.5 * t))}[kind]
    return f.astype(np.float32)


def voice(f0_true, T, K_sig, seed, noise=0.02, hop=HOP, sample_rate=SR):
    """A test voice (T samples, float64): harmonics 1..K_sig of the per-frame track f0_true with smooth random amplitude
    tracks of about 0.5 / k, plus white noise."""
    rng = np.random.default_rng(seed)
    F = len(f0_true)
    amps = 0.5 / np.arange(1, K_sig + 1) * (1 + 0.3 * np.sin(rng.uniform(0, 6.28, K_sig) + 0.2 * np.arange(F)[:, None]))
    y = bank(f0_true, amps, hop, sample_rate)
    y = np.concatenate([y, np.zeros(max(T - len(y), 0))])[:T]
    return y + noise * rng.normal(0, 1, T)


_cache = {}


def cases():
    """name -> (x fp32 (B, T), f0 fp32 (B, F), keyword arguments of ``analyse`` without ``fp32``): the inputs of the GPU test,
    which the host test runs through the fp32 stand-in.  The smallest shapes that reach each edge: B <= 3, T <= 4800."""
    if "cases" in _cache:
        return _cache["cases"]
    c = {}
    base = dict(sample_rate=SR, hop=HOP)

    def rows(tracks, T, K_sig, seed, hop=HOP, noise=0.02):
        return np.array([voice(np.asarray(tr, np.float64), T, K_sig, seed + n, noise, hop)
                         for n, tr in enumerate(tracks)]).astype(np.float32)

    # two rows, 11 frames: a glide and a vibrato, with unvoiced frames marked in the track handed to the analysis.  The
    # patterns take all four chirp rules, at the first and the last frame too
    F = 11
    true = [np.linspace(120.0, 180.0, F), 200.0 * 2 ** (0.04 * np.sin(np.arange(F)))]
    x2 = rows(true, 2400, 30, 100)
    f2 = np.array(true, np.float32)
    f2[0, [3, 5, 8, 9]] = 0      # v v v u v u v v u u v: forward, central, backward, none, forward, backward, none
    f2[1, [0, 1, 6]] = 0         # u u v v v v u v v v v: the first frame unvoiced, the last one backward
    for K in (1, 64, 65, 155, 256):
        c[f"K{K}"] = (x2, f2, dict(base, K=K, n_mag=65))
    for n_mag in (2, 65, 256, 257, 513):
        c[f"n_mag{n_mag}"] = (x2, f2, dict(base, K=8, n_mag=n_mag))
    c["no_noise"] = (x2, f2, dict(base, K=8, n_mag=0))
    for s in (1, 64):
        c[f"smooth{s}"] = (x2, f2, dict(base, K=8, n_mag=65, smooth=s))
    # the window at its extremes (one row each, 5 frames)
    for name, fz in (("L1600", 60.0), ("L_clamped", 40.0), ("L480_min_window", 1000.0), ("L_odd", 4 * SR / 961.0)):
        c[name] = (rows([np.full(5, fz)], 960, 10, 200), np.full((1, 5), fz, np.float32), dict(base, K=12, n_mag=33))
    xu = rows([np.full(5, 150.0)], 960, 10, 210, noise=0.2)
    fu = np.zeros((1, 5), np.float32)
    c["unvoiced_odd"] = (xu, fu, dict(base, K=4, n_mag=33, unvoiced_window=2047))
    c["unvoiced_limit"] = (xu, fu, dict(base, K=4, n_mag=33, unvoiced_window=2048))
    # one octave per 0.25 s
    Fg = 21
    steep = 100.0 * 2 ** (np.arange(Fg) * HOP / SR / 0.25)
    c["steep_glide"] = (rows([steep], 4800, 20, 300), steep.astype(np.float32)[None], dict(base, K=40, n_mag=65))
    # geometry
    c["T_lt_window"] = (rows([np.full(3, 100.0)], 500, 10, 400), np.full((1, 3), 100.0, np.float32),
                        dict(base, K=12, n_mag=33))
    c["F1"] = (rows([np.full(2, 150.0)], 100, 10, 410), np.full((1, 1), 150.0, np.float32), dict(base, K=12, n_mag=33))
    fm = np.full((1, 12), 100.0, np.float32)
    fm[0, 9] = 0
    c["more_frames"] = (rows([np.full(6, 100.0)], 1200, 10, 420), fm, dict(base, K=12, n_mag=33))   # frames 7.. read zeros
    th1 = np.linspace(900.0, 1100.0, 65)
    c["hop1"] = (rows([th1], 64, 5, 430, hop=1), th1.astype(np.float32)[None], dict(sample_rate=SR, hop=1, K=12, n_mag=33))
    th3 = np.linspace(110.0, 140.0, 9)
    c["hop300"] = (rows([th3, th3[::-1]], 2400, 20, 440, hop=300), np.array([th3, th3[::-1]], np.float32),
                   dict(sample_rate=SR, hop=300, K=30, n_mag=65))
    # the recipe's shape: B = 4, T = 4801, K = 155, n_mag = 256
    Fr = 4801 // HOP + 1
    tr = [np.linspace(80.0, 95.0, Fr), np.linspace(400.0, 300.0, Fr), 160.0 * 2 ** (0.03 * np.sin(0.7 * np.arange(Fr))),
          np.full(Fr, 220.0)]
    fr_ = np.array(tr, np.float32)
    fr_[2, 8:12] = 0
    fr_[3, :] = 0
    c["recipe"] = (rows(tr, 4801, 60, 500), fr_, dict(base, K=155, n_mag=256))
    _cache["cases"] = c
    return c


_ref_cache = {}


def reference(name):
    """The float64 result of a case, computed once and shared."""
    if name not in _ref_cache:
        x, f0, kw = cases()[name]
        _ref_cache[name] = analyse(x, f0, **kw)
    return _ref_cache[name]
