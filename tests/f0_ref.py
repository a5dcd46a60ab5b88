"""Float64 restatement of the f0 analysis (golf_f0_yin_f32, include/golf_amd.h): YIN steps 1-5, written from the definition
with numpy, one step after the other.  It is the checker of csrc/f0_yin.hip (tests/test_gpu_f0.py) and is itself pinned on
signals of known f0 by tests/test_f0_host.py.

``fp32=True`` is the rehearsal stand-in for the kernel's precision plan: the frame rounded to fp32, every difference,
square and sum of the difference function in fp32 (four partial sums over contiguous quarters of the window, as the
kernel's four waves keep them), the running sum in float64, d' rounded to fp32.  The host test holds it to the bars of the
GPU test against the float64 version, on the GPU test's own inputs.

Also here: the signals and the cases both test files share."""
import math

import numpy as np


def lags(sample_rate, f0_min=60.0, f0_max=1000.0, window_length=None):
    tau_min, tau_max = int(math.floor(sample_rate / f0_max)), int(math.ceil(sample_rate / f0_min))
    return tau_min, tau_max, 2 * tau_max if window_length is None else int(window_length)


def n_frames(T, S, hop, centred=True):
    return T // hop + 1 if centred else max(T - S, 0) // hop + 1


def frames(x, hop, S, origin, F):
    """(B, F, S): s[b, f, k] = x[b, origin + f*hop + k], zero outside [0, T)."""
    T = x.shape[1]
    idx = origin + np.arange(F)[:, None] * hop + np.arange(S)[None, :]
    ok = (idx >= 0) & (idx < T)
    if T == 0:
        return np.zeros((x.shape[0], F, S), x.dtype)
    return np.where(ok[None], x[:, np.clip(idx, 0, T - 1)], 0).astype(x.dtype)


def yin(x, sample_rate, hop, W, tau_min, tau_max, threshold=0.15, rms_floor=0.0, centred=True, F=None, fp32=False):
    """x (B, T) -> dict of (B, F) arrays: f0, period, ap (float64), tau (integer lag tau*), first (the first lag below the
    threshold, -1 if none), found, voiced; and dprime (B, F, tau_max + 1)."""
    x = np.asarray(x)
    assert x.ndim == 2 and hop >= 1 and 1 <= tau_min < tau_max and W >= 1
    S = W + tau_max
    F = n_frames(x.shape[1], S, hop, centred) if F is None else F
    dt = np.float32 if fp32 else np.float64
    s = frames(x.astype(dt), hop, S, -(S // 2) if centred else 0, F)
    B = s.shape[0]

    # 1. difference function
    d = np.zeros((B, F, tau_max + 1), dt)
    cuts = [0, W] if not fp32 else [(W // 8 * q // 4) * 8 for q in range(4)] + [W]
    for tau in range(tau_max + 1):
        diff = s[..., :W] - s[..., tau:tau + W]
        sq = diff * diff
        acc = np.zeros((B, F), dt)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            acc = acc + sq[..., lo:hi].sum(-1, dtype=dt)
        d[..., tau] = acc
    # 2. cumulative-mean normalisation
    run = np.cumsum(d[..., 1:].astype(np.float64), -1)
    dprime = np.ones((B, F, tau_max + 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        dprime[..., 1:] = np.where(run != 0, d[..., 1:].astype(np.float64) * np.arange(1, tau_max + 1) / run, 1.0)
    if fp32:
        dprime = dprime.astype(np.float32).astype(np.float64)

    out = {k: np.zeros((B, F)) for k in ("f0", "period", "ap")}
    out.update(tau=np.zeros((B, F), int), first=np.full((B, F), -1), found=np.zeros((B, F), bool),
               voiced=np.zeros((B, F), bool), dprime=dprime)
    for b in range(B):
        for f in range(F):
            dp = dprime[b, f]
            # 3. search
            below = np.nonzero(dp[tau_min:tau_max + 1] < threshold)[0]
            found = below.size > 0
            if found:
                t = first = tau_min + int(below[0])
                while t + 1 <= tau_max and dp[t + 1] < dp[t]:
                    t += 1
            else:
                t, first = tau_min + int(np.argmin(dp[tau_min:tau_max + 1])), -1   # argmin: the first of equal minima
            # 4. parabolic refinement
            delta, ap = 0.0, dp[t]
            if t - 1 >= 1 and t + 1 <= tau_max:
                a_, b_, c_ = dp[t - 1], dp[t], dp[t + 1]
                if a_ - 2 * b_ + c_ > 0:
                    delta = min(max((a_ - c_) / (2 * (a_ - 2 * b_ + c_)), -1.0), 1.0)
                    ap = b_ - (a_ - c_) * delta / 4
            period = t + delta
            # 5. voicing
            voiced = found and float(np.mean(s[b, f, :W].astype(np.float64) ** 2)) > rms_floor ** 2
            out["tau"][b, f], out["first"][b, f], out["found"][b, f], out["voiced"][b, f] = t, first, found, voiced
            out["period"][b, f], out["ap"][b, f] = period, ap
            out["f0"][b, f] = sample_rate / period if voiced else 0.0
    return out


# ---- signals -------------------------------------------------------------------------------------------------------------
def tone(f0, T, sr, harmonics=10):
    """Harmonics 1..10 of f0 with amplitudes 1/h and phases h (those below Nyquist)."""
    t = np.arange(T) / sr
    return sum(np.sin(2 * np.pi * f0 * h * t + h) / h for h in range(1, harmonics + 1) if f0 * h < sr / 2)


def glide(f_lo, f_hi, T, sr, harmonics=10):
    """A linear glide of the fundamental; returns (signal, instantaneous f0 per sample)."""
    f = np.linspace(f_lo, f_hi, T)
    ph = np.cumsum(f / sr)
    return sum(np.sin(2 * np.pi * h * ph) / h for h in range(1, harmonics + 1)), f


RECIPE = dict(sr=24000.0, hop=240, W=1024, f0_min=60.0, f0_max=1000.0, threshold=0.15, T=4801)
RECIPE_TONES = (80.0, 150.3, 440.0, 900.0)
_cache = {}


def recipe_rows():
    """The eight rows of the recipe case, fp32 (8, 4801): four tones, noise, a tone with a zeroed stretch, a tone in noise,
    a glide.  Also returns the glide's instantaneous f0."""
    if "rows" not in _cache:
        T, sr = RECIPE["T"], RECIPE["sr"]
        rng = np.random.default_rng(2002)
        rows = [tone(f, T, sr) for f in RECIPE_TONES]
        rows.append(rng.normal(0, 1, T))
        gap = tone(150.3, T, sr)
        gap[1500:3500] = 0
        rows.append(gap)
        rows.append(tone(150.3, T, sr) + 0.3 * rng.normal(0, 1, T))
        g, fg = glide(140.0, 180.0, T, sr)
        rows.append(g)
        _cache["rows"] = (np.array(rows).astype(np.float32), fg)
    return _cache["rows"]


def small_rows(B, T, sr, seed):
    """Tone and noise rows in turn, for the small cases."""
    rng = np.random.default_rng(seed)
    f0s = np.geomspace(sr / 30.0, sr / 6.0, B)
    return np.array([tone(f0s[i], T, sr, 4) + 0.01 * rng.normal(0, 1, T) if i % 2 == 0 else rng.normal(0, 1, T)
                     for i in range(B)]).astype(np.float32)


def cases():
    """name -> (x fp32 (B, T), keyword arguments of ``yin`` without ``fp32``): the inputs of the GPU test, which the host
    test runs through the fp32 stand-in."""
    if "cases" in _cache:
        return _cache["cases"]
    c = {}
    tmin, tmax, W = lags(RECIPE["sr"], RECIPE["f0_min"], RECIPE["f0_max"], RECIPE["W"])
    rec = dict(sample_rate=RECIPE["sr"], hop=RECIPE["hop"], W=W, tau_min=tmin, tau_max=tmax, threshold=RECIPE["threshold"])
    rows = recipe_rows()[0]
    c["recipe"] = (rows, rec)
    c["edges"] = (rows[[1, 4, 7], 1700:2700], rec)                          # T = 1000 < S = 1424: padded on both sides
    sm = dict(sample_rate=8000.0, hop=7, tau_min=4, tau_max=40, threshold=0.15)
    xs = small_rows(5, 777, 8000.0, 50)
    c["small50"] = (xs, dict(sm, W=50))
    c["small51"] = (xs, dict(sm, W=51))
    c["hop_gt_W"] = (xs, dict(sm, hop=200, W=128))
    c["S_gt_T"] = (xs[:, :100], dict(sm, W=256))
    c["from0"] = (xs, dict(sm, W=50, centred=False))
    c["more_frames"] = (xs[:2], dict(sm, W=50, F=777 // 7 + 1 + 12))        # the frames from 118 on read only zeros
    # lag tile edges: 256 lags a tile (tau_max + 1 = 256, 257), and the 64-lag steps of the scan and of the search
    xl = small_rows(3, 900, 8000.0, 51)
    for tm in (63, 64, 65, 127, 128, 129, 254, 255, 256, 257, 511, 512):
        c[f"tau_max{tm}"] = (xl, dict(sample_rate=8000.0, hop=300, W=77, tau_min=4, tau_max=tm, threshold=0.15))
    rng = np.random.default_rng(52)
    big = (tone(3.1, 20000, 8000.0, 6) + 0.05 * rng.normal(0, 1, 20000)).astype(np.float32)[None]
    c["largest"] = (big, dict(sample_rate=8000.0, hop=12000, W=8190, tau_min=20, tau_max=8194, threshold=0.15))   # S = 16384
    # search branches (sr 8000, lags 4 .. 40)
    t = np.arange(777) / 8000.0
    c["first_at_tau_min"] = (np.sin(2 * np.pi * 2000.0 * t + 0.3).astype(np.float32)[None], dict(sm, W=50))
    c["star_at_tau_max"] = (np.sin(2 * np.pi * 200.0 * t + 0.3).astype(np.float32)[None], dict(sm, W=50))
    c["walk"] = (tone(330.0, 777, 8000.0, 3).astype(np.float32)[None], dict(sm, W=50, threshold=0.6))
    c["fallback"] = (xs[1:2], dict(sm, W=50))
    quiet = (1e-3 * tone(400.0, 777, 8000.0, 4)).astype(np.float32)[None]
    c["quiet"] = (quiet, dict(sm, W=50))
    c["quiet_floor"] = (quiet, dict(sm, W=50, rms_floor=0.01))
    _cache["cases"] = c
    return c


_ref_cache = {}


def reference(name):
    """The float64 result of a case, computed once and shared."""
    if name not in _ref_cache:
        x, kw = cases()[name]
        _ref_cache[name] = yin(x, **kw)
    return _ref_cache[name]
