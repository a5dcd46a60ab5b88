"""Float64 restatement of the spectral-envelope analysis (golf_spectral_envelope_f32, include/golf_amd.h), written from the
definition with numpy, steps 1 to 8 one after the other.  It is the checker of csrc/spec_envelope.hip (tests/test_gpu_env.py)
and is itself pinned on signals with a planted envelope by tests/test_env_host.py.

``fp32=True`` is the stand-in for a plain fp32 kernel: the frame constants still in float64, the window, the windowed
samples, the three transforms (a radix-2 Stockham FFT in complex64 with fp32 twiddles), the interpolation, the smoothing
sums, the log and the lifter in float32.  The host test holds it to the bars of the GPU test against the float64 version, on
the GPU test's own inputs.

Also here: the signals and the cases both test files share."""
import math

import numpy as np

SR, HOP, N_FFT = 24000.0, 240, 1024
OFFSET = 0.5 * math.log(2.0)    # the default voiced_offset
DB = 20.0 / math.log(10.0)      # nepers -> dB


def defaults(sample_rate, n_fft, f0_floor=None, f0_ceil=None):
    return (3.0 * sample_rate / (n_fft - 3) if f0_floor is None else float(f0_floor),
            sample_rate / 12.0 if f0_ceil is None else float(f0_ceil))


def frame_constants(f0v, sample_rate, n_fft, f0_floor, f0_ceil, unvoiced_f0):
    """Steps 1 and 2 in float64 from the fp32 value: (voiced, fe, hw, r0, r)."""
    fd = float(f0v)
    voiced = fd > 0   # False for a NaN
    fe = min(max(fd, f0_floor), f0_ceil) if voiced else float(unvoiced_f0)
    hw = int(math.floor(1.5 * sample_rate / fe + 0.5))
    r0 = fe * n_fft / sample_rate
    return voiced, fe, hw, r0, r0 / 3.0


def _fft(a, fp32):
    """The forward DFT of a length-n vector.  fp32: radix-2 Stockham in complex64, twiddles exp(-2 pi j k / n) rounded to
    fp32, as an LDS FFT forms it."""
    if not fp32:
        return np.fft.fft(a.astype(np.complex128))
    n = len(a)
    a = a.astype(np.complex64)
    tw = np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64)
    j = np.arange(n // 2)
    ns = 1
    while ns < n:
        k = j & (ns - 1)
        u0, u1 = a[j], (a[j + n // 2] * tw[k * (n // (2 * ns))]).astype(np.complex64)
        out = np.empty(n, np.complex64)
        j0 = ((j - k) << 1) + k
        out[j0], out[j0 + ns] = u0 + u1, u0 - u1
        a, ns = out, 2 * ns
    return a


def _even(h):
    """c_0 .. c_{n/2} -> its even extension of length n."""
    return np.concatenate([h, h[-2:0:-1]])


def smooth(P, r, dt=np.float64):
    """Step 5: the mean over [k - r, k + r] of the piecewise-constant, evenly extended spectrum P (bins 0 .. n/2)."""
    nh = len(P) - 1
    D = int(math.ceil(r)) + 1
    k = np.arange(nh + 1, dtype=np.float64)[:, None]
    j = k + np.arange(-D, D + 1, dtype=np.float64)[None, :]
    lo, hi = k - r, k + r
    wgt = np.clip(np.minimum(hi, j + 0.5) - np.maximum(lo, j - 0.5), 0.0, None)   # the covered part of cell j
    ji = np.abs(j.astype(int))
    ji = np.where(ji > nh, 2 * nh - ji, ji)
    acc = (wgt.astype(dt) * P.astype(dt)[ji]).sum(1, dtype=dt)
    return (acc / dt(2.0 * r)).astype(dt)


def analyse_frame(seg, fe, hw, r0, r, sample_rate, n_fft, q1, eps, fp32=False):
    """Steps 2 to 7 on the samples seg = x[f hop - hw .. f hop + hw]: (c' (n/2 + 1), P, Ps)."""
    dt = np.float32 if fp32 else np.float64
    n, nh = n_fft, n_fft // 2
    m = np.arange(-hw, hw + 1)
    arg = m.astype(np.float64) * fe / (3.0 * sample_rate)
    w = (0.5 + 0.5 * np.cos(2 * np.pi * arg)).astype(dt)
    xw = (w * seg.astype(dt)).astype(dt)
    sum_w, sum_w2, sum_xw = w.sum(dtype=dt), (w * w).sum(dtype=dt), xw.sum(dtype=dt)
    xw = (xw - w * dt(sum_xw / sum_w)).astype(dt)
    buf = np.zeros(n, dt)
    buf[m % n] = xw
    X = _fft(buf, fp32)[:nh + 1]
    P = ((X.real.astype(dt) ** 2 + X.imag.astype(dt) ** 2) / sum_w2).astype(dt)
    # step 4
    Pc = P.copy()
    kk = np.arange(nh + 1)
    low = kk[kk < r0]
    u = r0 - low
    i0 = np.floor(u).astype(int)
    t = (u - i0).astype(dt)
    i1 = np.minimum(i0 + 1, nh)
    Pc[low] = (P[low] + ((dt(1) - t) * P[i0] + t * P[i1])).astype(dt)
    # step 5, 6
    Ps = smooth(Pc, r, dt)
    L = np.log((Ps + dt(eps)).astype(dt)).astype(dt)
    c = (_fft(_even(L), fp32).real[:nh + 1].astype(dt) / dt(n)).astype(dt)
    # step 7
    q = np.arange(nh + 1, dtype=np.float64)
    tq = fe * q / sample_rate
    sinc = np.where(q == 0, 1.0, np.sin(np.pi * tq) / np.where(q == 0, 1.0, np.pi * tq))
    lift = sinc * ((1 - 2 * q1) + 2 * q1 * np.cos(2 * np.pi * tq))
    return (c * lift.astype(dt)).astype(dt), P, Ps


def analyse(x, f0, sample_rate, hop, n_fft=N_FFT, n_ceps=None, f0_floor=None, f0_ceil=None, unvoiced_f0=500.0, q1=-0.15,
            eps=1e-12, voiced_offset=OFFSET, fp32=False):
    """x (B, T), f0 (B, F) -> dict: log_env (B, F, n/2 + 1), ceps (B, F, n_ceps; n/2 + 1 when None) and per frame voiced,
    fe, hw, r0, r."""
    x, f0 = np.asarray(x), np.asarray(f0)
    assert x.ndim == 2 and f0.ndim == 2 and x.shape[0] == f0.shape[0]
    n, nh = int(n_fft), int(n_fft) // 2
    f0_floor, f0_ceil = defaults(sample_rate, n, f0_floor, f0_ceil)
    n_ceps = nh + 1 if n_ceps is None else n_ceps
    assert 0 < f0_floor <= unvoiced_f0 <= f0_ceil <= sample_rate / 4 and 0 <= n_ceps <= nh + 1
    assert math.floor(1.5 * sample_rate / f0_floor + 0.5) <= nh - 1
    (B, T), F = x.shape, f0.shape[1]
    dt = np.float32 if fp32 else np.float64
    log_env, ceps = np.zeros((B, F, nh + 1)), np.zeros((B, F, n_ceps))
    info = {k: np.zeros((B, F), t) for k, t in (("voiced", bool), ("fe", float), ("hw", int), ("r0", float), ("r", float))}
    for b in range(B):
        for f in range(F):
            voiced, fe, hw, r0, r = frame_constants(f0[b, f], sample_rate, n, f0_floor, f0_ceil, unvoiced_f0)
            for k, v in zip(("voiced", "fe", "hw", "r0", "r"), (voiced, fe, hw, r0, r)):
                info[k][b, f] = v
            t = f * hop + np.arange(-hw, hw + 1)
            ok = (t >= 0) & (t < T)
            seg = np.where(ok, x[b, np.clip(t, 0, max(T - 1, 0))] if T else 0.0, 0.0)
            cl, _, _ = analyse_frame(seg, fe, hw, r0, r, float(sample_rate), n, q1, eps, fp32)
            off = dt(voiced_offset if voiced else 0.0)
            env = (dt(0.5) * _fft(_even(cl), fp32).real[:nh + 1].astype(dt) + off).astype(dt)
            cp = (dt(0.5) * cl[:n_ceps]).astype(dt)
            if n_ceps:
                cp[0] = cp[0] + off
            log_env[b, f], ceps[b, f] = env, cp
    return dict(log_env=log_env, ceps=ceps, **info)


def errors(out, ref):
    """The largest errors of ``out`` against ``ref`` in the GPU test's units: magnitudes exp(log_env) in units of the frame's
    largest reference magnitude, and ceps in nepers."""
    mag = np.exp(ref["log_env"])
    e_env = (np.abs(np.exp(out["log_env"]) - mag) / mag.max(-1, keepdims=True)).max(initial=0.0)
    nc = min(out["ceps"].shape[-1], ref["ceps"].shape[-1])
    e_ceps = np.abs(out["ceps"][..., :nc] - ref["ceps"][..., :nc]).max(initial=0.0)
    return e_env, e_ceps


# ---- signals -------------------------------------------------------------------------------------------------------------
PLANTED_CEPS = np.array([-1.0, 0.6, -0.3, 0.2, 0.1, -0.15, 0.05])


def log_response(ceps, freq):
    """log|H| at the frequencies ``freq`` (cycles per sample) in LTVCepFilter's convention: c_0 + 2 sum c_m cos(2 pi f m)."""
    m = np.arange(1, len(ceps))
    return ceps[0] + 2.0 * np.cos(2 * np.pi * np.multiply.outer(freq, m)) @ ceps[1:]


def upsample(z, hop):
    """Linear upsampling of the frames z (F) to (F-1)*hop + 1 samples, as the oscillator bank upsamples its controls."""
    F = len(z)
    pos = np.arange((F - 1) * hop + 1) / hop
    lo = np.minimum(pos.astype(int), max(F - 2, 0))
    fr = pos - lo
    return z[lo] * (1 - fr) + z[np.minimum(lo + 1, F - 1)] * fr


def pulse_voice(f0, hop, sample_rate, ceps=PLANTED_CEPS, noise=1e-3, seed=0, phase0=None):
    """Harmonics sqrt(2 f0 / sr) |H(k f0)| sin(2 pi k phi) up to Nyquist (the pulse train of AdditivePulseTrain through the
    envelope planted by ``ceps``), plus white noise of standard deviation ``noise``: (F-1)*hop + 1 samples in float64.
    f0 (F) in Hz per frame; ``phase0`` (cycles per harmonic) starts the harmonics elsewhere than 0."""
    p = upsample(np.asarray(f0, np.float64), hop) / sample_rate
    phi = np.cumsum(p)
    y = np.zeros(len(p))
    for k in range(1, int(0.5 / p.min()) + 1):
        live = k * p < 0.5
        ph0 = 0.0 if phase0 is None else phase0[k % len(phase0)]
        y += live * np.sqrt(2 * p) * np.exp(log_response(ceps, k * p)) * np.sin(2 * np.pi * (k * phi + ph0))
    if noise:
        y = y + noise * np.random.default_rng(seed).normal(0, 1, len(y))
    return y


def recovery_errors(out, ceps=PLANTED_CEPS, drop=5, top=0.95):
    """(max, rms, mean) error in dB of row 0's log_env against the planted envelope: interior frames, bins below ``top`` of
    Nyquist."""
    env = out["log_env"][0]
    nb = env.shape[-1]
    nk = int(math.ceil(top * (nb - 1)))
    want = log_response(ceps, np.arange(nk) / (2.0 * (nb - 1)))
    d = DB * (env[drop:len(env) - drop, :nk] - want)
    return np.abs(d).max(), math.sqrt((d * d).mean()), d.mean()


# ---- the cases of the GPU test -------------------------------------------------------------------------------------------
_cache = {}


def _rows(tracks, hop, sample_rate, T, seed):
    """fp32 rows: the pulse voice of each track through the planted envelope, faded out over its unvoiced, NaN and negative
    frames (a row without a voiced frame is white noise), plus white noise 60 dB below the row's rms, cut or zero-padded to
    T samples."""
    rows = []
    for i, tr in enumerate(tracks):
        tr = np.asarray(tr, np.float64)
        sound = np.where(tr > 0, tr, 0.0)
        if (sound > 0).any():
            fill = np.where(sound > 0, sound, sound[sound > 0].mean())
            y = pulse_voice(np.minimum(fill, 0.24 * sample_rate), hop, sample_rate, noise=0.0,
                            phase0=np.random.default_rng(seed + i).uniform(0, 1, 7))
            y = y * upsample((sound > 0).astype(np.float64), hop)
        else:
            y = np.random.default_rng(seed + i).normal(0, 0.1, (len(tr) - 1) * hop + 1)
        y = np.concatenate([y, np.zeros(max(T - len(y), 0))])[:T]
        rms = math.sqrt((y * y).mean()) if T else 0.0
        rows.append(y + 1e-3 * rms * np.random.default_rng(seed + 50 + i).normal(0, 1, T))
    return np.array(rows).astype(np.float32).reshape(len(tracks), T)


def cases():
    """name -> (x fp32 (B, T), f0 fp32 (B, F), keyword arguments of ``analyse`` without ``fp32``): the inputs of the GPU test,
    which the host test runs through the fp32 stand-in.  B = 3, F of 8 to 12; the sample rate is scaled with n_fft so that the
    windows fit."""
    if "cases" in _cache:
        return _cache["cases"]
    c = {}

    def make(name, n, hop, tracks, T=None, seed=0, **kw):
        sr = SR * n / 1024
        tracks = np.array(tracks, np.float32)
        T = (tracks.shape[1] - 1) * hop + 1 if T is None else T
        c[name] = (_rows(tracks, hop, sr, T, seed), tracks, dict(dict(sample_rate=sr, hop=hop, n_fft=n), **kw))

    def voices(n):
        """Three voiced tracks inside [f0_floor, f0_ceil] of the transform size (the recipe's: speech-like)."""
        if n == 1024:
            return [np.linspace(110.0, 180.0, 9), np.linspace(420.0, 300.0, 9), np.full(9, 233.0)]
        lo, hi = defaults(SR * n / 1024, n)
        return [np.linspace(1.1 * lo, 0.5 * (lo + hi), 9), np.linspace(0.95 * hi, 0.6 * hi, 9), np.full(9, math.sqrt(lo * hi))]

    def mid(n):
        return math.sqrt(np.prod(defaults(SR * n / 1024, n)))

    # the four transform sizes on plain voiced rows
    make("n64", 64, 8, voices(64), seed=10, unvoiced_f0=mid(64))
    make("n256", 256, 60, voices(256), seed=20, unvoiced_f0=mid(256))
    make("n1024", 1024, 240, voices(1024), seed=30)
    make("n2048", 2048, 480, voices(2048), seed=40, unvoiced_f0=mid(2048))
    # log2 n odd, like 2048: the kernel's ping-pong FFT ends in the other buffer
    make("n128", 128, 15, voices(128), seed=15, unvoiced_f0=mid(128))
    make("n512", 512, 120, voices(512), seed=25, unvoiced_f0=mid(512))
    # the clamps: f0 below f0_floor (the longest window) and above f0_ceil (the shortest), and one in between
    make("clamps", 1024, 240, [np.full(8, 50.0), np.full(8, 2500.0), np.full(8, 300.0)], seed=50)
    make("floor_1021", 1024, 240, [np.full(8, 40.0), np.full(8, 60.0), np.full(8, 70.0)], seed=55,
         f0_floor=3 * SR / 1020.5)   # hw = 510: 2 hw + 1 = n_fft - 3
    # r an exact integer and an exact half-integer: fe = 3 sr r / n
    make("cell_edges", 1024, 240, [np.full(8, 140.625), np.full(8, 175.78125), np.full(8, 210.9375)], seed=70)
    # unvoiced, NaN and negative f0 beside voiced frames
    mixed = [[150, 0, 160, np.nan, 170, -100, 180, 185, 0, 0, 190, 200],
             [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
             [np.nan, 220, 220, 220, -1, 220, 220, 0, 220, 220, 220, np.nan]]
    make("mixed", 1024, 240, mixed, seed=80)
    # geometry: T shorter than one window (the later frames read no sample), and no sample at all
    make("T_short", 1024, 240, voices(1024), T=150, seed=90)
    make("T0", 1024, 240, voices(1024), T=0, seed=95)
    # the outputs' widths
    make("n_ceps1", 1024, 240, voices(1024), seed=30, n_ceps=1)
    make("n_ceps241", 1024, 240, voices(1024), seed=30, n_ceps=241)
    _cache["cases"] = c
    return c


_ref_cache = {}


def reference(name):
    """The float64 result of a case, computed once and shared."""
    if name not in _ref_cache:
        x, f0, kw = cases()[name]
        _ref_cache[name] = analyse(x, f0, **kw)
    return _ref_cache[name]
