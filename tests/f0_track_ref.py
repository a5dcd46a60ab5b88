"""Float64 restatement of the f0 tracker (golf_f0_candidates_f32 and golf_f0_viterbi_f32, include/golf_amd.h), written from
the definition with plain loops: candidates from the d' of ``f0_ref.yin`` (``fp32=True`` gives the stand-in of the kernel's
precision plan), the path search, the cost of a given path, and ``margin`` -- the smallest gap between the best and the
second-best predecessor over every (frame, state) and between the best and the second-best end state: above roundoff the
path is unique, so a kernel that computes the same costs to 1e-12 must return the same states.

Also here: the signals, the cases and the error count that tests/test_f0_track_host.py and tests/test_gpu_f0_track.py share.
It is the checker of csrc/f0_viterbi.hip and of the candidate kernel in csrc/f0_yin.hip."""
import itertools
import math

import numpy as np

import f0_ref as R

COSTS = dict(unvoiced_cost=0.3, lag_cost=0.02, jump_cost=0.35, switch_cost=0.14)   # the defaults of functional.f0_viterbi


# ---- candidates ----------------------------------------------------------------------------------------------------------
def candidates(x, sample_rate, hop, W, tau_min, tau_max, K=7, rms_floor=0.0, centred=True, F=None, fp32=False, threshold=0.15,
               yin=None):
    """x (B, T) -> dict: period, ap (B, F, K) float64 with absent slots 0 / +inf, lag (B, F, K) integer lags with -1 for
    absent slots, n_minima (B, F) the number of local minima before the selection, and yin, the result of ``f0_ref.yin`` on
    the same frames (``threshold`` only matters to that; ``yin`` hands in one computed before, for its d')."""
    y = yin if yin is not None else R.yin(x, sample_rate, hop, W, tau_min, tau_max, threshold=threshold, rms_floor=rms_floor,
                                          centred=centred, F=F, fp32=fp32)
    dprime = y["dprime"]
    B, F = dprime.shape[:2]
    S = W + tau_max
    s = R.frames(np.asarray(x).astype(np.float32 if fp32 else np.float64), hop, S, -(S // 2) if centred else 0, F)
    period, ap = np.zeros((B, F, K)), np.full((B, F, K), np.inf)
    lag, n_minima = np.full((B, F, K), -1), np.zeros((B, F), int)
    for b in range(B):
        for f in range(F):
            dp = dprime[b, f]
            minima = [t for t in range(tau_min, tau_max + 1)
                      if dp[t] < dp[t - 1] and (t == tau_max or dp[t] <= dp[t + 1])]
            n_minima[b, f] = len(minima)
            if float(np.mean(s[b, f, :W].astype(np.float64) ** 2)) <= rms_floor ** 2:
                continue
            kept = sorted(sorted(minima, key=lambda t: (dp[t], t))[:K])
            for k, t in enumerate(kept):
                delta, a = 0.0, dp[t]
                if t - 1 >= 1 and t + 1 <= tau_max:
                    a_, b_, c_ = dp[t - 1], dp[t], dp[t + 1]
                    if a_ - 2 * b_ + c_ > 0:
                        delta = min(max((a_ - c_) / (2 * (a_ - 2 * b_ + c_)), -1.0), 1.0)
                        a = b_ - (a_ - c_) * delta / 4
                period[b, f, k], ap[b, f, k], lag[b, f, k] = t + delta, a, t
    return dict(period=period, ap=ap, lag=lag, n_minima=n_minima, yin=y)


# ---- path search ---------------------------------------------------------------------------------------------------------
def present(period, ap):
    return (period > 0) & ~np.isnan(ap) & ~(ap == np.inf)


def _local(p, a, lag_ref, unvoiced_cost, lag_cost):
    """Local costs of one frame: list of 1 + K entries, None for an absent state."""
    out = [unvoiced_cost]
    for k in range(len(p)):
        ok = p[k] > 0 and not math.isnan(a[k]) and a[k] != math.inf
        out.append(max(a[k], 0.0) + lag_cost * (math.log2(p[k]) - math.log2(lag_ref)) if ok else None)
    return out


def _trans(i, j, p_prev, p_now, jump_cost, switch_cost):
    if i == 0 and j == 0:
        return 0.0
    if i == 0 or j == 0:
        return switch_cost
    return jump_cost * abs(math.log2(p_now[j - 1]) - math.log2(p_prev[i - 1]))


def viterbi_row(period, ap, sample_rate, lag_ref, unvoiced_cost=0.3, lag_cost=0.02, jump_cost=0.35, switch_cost=0.14):
    """period, ap (F, K) -> (state (F,), f0 (F,), cost, margin) of one utterance."""
    period, ap = np.asarray(period, np.float64), np.asarray(ap, np.float64)
    F, K = period.shape
    margin = math.inf
    loc = _local(period[0], ap[0], lag_ref, unvoiced_cost, lag_cost)
    C = list(loc)
    back = np.zeros((F, K + 1), int)
    for f in range(1, F):
        loc = _local(period[f], ap[f], lag_ref, unvoiced_cost, lag_cost)
        new = [None] * (K + 1)
        for j in range(K + 1):
            if loc[j] is None:
                continue
            best, arg, second = math.inf, -1, math.inf
            for i in range(K + 1):
                if C[i] is None:
                    continue
                v = C[i] + _trans(i, j, period[f - 1], period[f], jump_cost, switch_cost)
                if v < best:
                    best, arg, second = v, i, best
                elif v < second:
                    second = v
            margin = min(margin, second - best)
            new[j], back[f, j] = loc[j] + best, arg
        C = new
    best, arg, second = math.inf, -1, math.inf
    for s_ in range(K + 1):
        if C[s_] is None:
            continue
        if C[s_] < best:
            best, arg, second = C[s_], s_, best
        elif C[s_] < second:
            second = C[s_]
    margin = min(margin, second - best)
    state = np.zeros(F, int)
    state[F - 1] = arg
    for f in range(F - 1, 0, -1):
        state[f - 1] = back[f, state[f]]
    f0 = np.array([sample_rate / period[f, s_ - 1] if s_ > 0 else 0.0 for f, s_ in enumerate(state)])
    return state, f0, best, margin


def viterbi(period, ap, sample_rate, lag_ref, **costs):
    """(B, F, K) -> dict: state (B, F) int, f0 (B, F), cost (B,), margin (the smallest over the rows)."""
    rows = [viterbi_row(period[b], ap[b], sample_rate, lag_ref, **costs) for b in range(len(period))]
    return dict(state=np.array([r[0] for r in rows]), f0=np.array([r[1] for r in rows]),
                cost=np.array([r[2] for r in rows]), margin=min([r[3] for r in rows], default=math.inf))


def path_cost(state, period, ap, lag_ref, unvoiced_cost=0.3, lag_cost=0.02, jump_cost=0.35, switch_cost=0.14):
    """The cost of the state path of one utterance, +inf if it enters an absent state (or one that does not exist)."""
    period, ap = np.asarray(period, np.float64), np.asarray(ap, np.float64)
    F, K = period.shape
    total = 0.0
    for f in range(F):
        s_ = int(state[f])
        if not 0 <= s_ <= K:
            return math.inf
        loc = _local(period[f], ap[f], lag_ref, unvoiced_cost, lag_cost)
        if loc[s_] is None:
            return math.inf
        total += loc[s_]
        if f > 0:
            total += _trans(int(state[f - 1]), s_, period[f - 1], period[f], jump_cost, switch_cost)
    return total


def brute_force(period, ap, lag_ref, **costs):
    """Every path of a small utterance: (the cheapest cost, the paths that reach it within 1e-12)."""
    F, K = np.asarray(period).shape
    all_costs = [(path_cost(p, period, ap, lag_ref, **costs), p) for p in itertools.product(range(K + 1), repeat=F)]
    best = min(c for c, _ in all_costs)
    return best, [p for c, p in all_costs if c <= best + 1e-12]


# ---- signals and cases ---------------------------------------------------------------------------------------------------
H_A1 = (0.2, 0.3, 0.4)
_cache = {}


def signal_h(a1):
    """A 120 Hz voice with a weak, amplitude-modulated fundamental and a strong second harmonic, fp32 (1, 4801)."""
    T, sr = R.RECIPE["T"], R.RECIPE["sr"]
    t = np.arange(T) / sr
    am = 1 + 0.5 * np.sin(2 * np.pi * 7 * t)
    x = (a1 * np.sin(2 * np.pi * 120 * t) * am + np.sin(2 * np.pi * 240 * t + 1) + 0.3 * np.sin(2 * np.pi * 360 * t + 2) * am
         + 0.02 * np.random.default_rng(int(a1 * 100)).normal(0, 1, T))
    return x.astype(np.float32)[None]


def noisy_rows():
    """The 150.3 Hz tone and the 140 -> 180 Hz glide of the recipe in white noise of sigma 0.4, fp32 (2, 4801); and the
    glide's instantaneous f0."""
    T, sr = R.RECIPE["T"], R.RECIPE["sr"]
    rng = np.random.default_rng(40)
    g, fg = R.glide(140.0, 180.0, T, sr)
    rows = [R.tone(150.3, T, sr) + 0.4 * rng.normal(0, 1, T), g + 0.4 * rng.normal(0, 1, T)]
    return np.array(rows).astype(np.float32), fg


def recipe_kw():
    tmin, tmax, W = R.lags(R.RECIPE["sr"], R.RECIPE["f0_min"], R.RECIPE["f0_max"], R.RECIPE["W"])
    return dict(sample_rate=R.RECIPE["sr"], hop=R.RECIPE["hop"], W=W, tau_min=tmin, tau_max=tmax)


def truth(name):
    """True f0 per frame (0 = unvoiced) of the end-to-end cases, (B, F)."""
    F = R.RECIPE["T"] // R.RECIPE["hop"] + 1
    if name.startswith("H"):
        return np.full((1, F), 120.0)
    if name == "noisy":
        fg = noisy_rows()[1]
        return np.stack([np.full(F, 150.3), fg[np.minimum(np.arange(F) * R.RECIPE["hop"], len(fg) - 1)]])
    raise KeyError(name)


def gross_errors(f0, true):
    """Per row the number of gross errors on frames 3 .. F-4: a voiced truth missed (f0 == 0) or off by more than 20 %, an
    unvoiced truth called voiced."""
    f0, true = np.asarray(f0, np.float64)[:, 3:-3], np.asarray(true, np.float64)[:, 3:-3]
    bad = np.where(true > 0, (f0 == 0) | (np.abs(f0 - true) > 0.2 * true), f0 > 0)
    return bad.sum(1)


def e2e_cases():
    """name -> (x fp32 (B, T), keyword arguments): signals H and the noisy rows at the recipe's analysis."""
    if "e2e" not in _cache:
        c = {f"H{a1}": (signal_h(a1), recipe_kw()) for a1 in H_A1}
        c["noisy"] = (noisy_rows()[0], recipe_kw())
        _cache["e2e"] = c
    return _cache["e2e"]


CAND_CASES = ("recipe", "edges", "small50", "small51", "from0", "more_frames", "hop_gt_W", "S_gt_T", "largest",
              "star_at_tau_max", "first_at_tau_min", "fallback", "quiet_floor")


def cand_case_names():
    """The cases of ``f0_ref.cases()`` that the candidate kernel is held to, every tau_max* case among them."""
    return [n for n in R.cases() if n in CAND_CASES or n.startswith("tau_max")]


PATH_CASES = ("recipe", "edges", "small50", "small51", "from0", "tau_max257", "walk")   # path equality is demanded on these


_ref = {}


def cand_reference(name, K):
    """Float64 candidates of a case, computed once and shared."""
    if (name, K) not in _ref:
        x, kw = (R.cases()[name] if name in R.cases() else e2e_cases()[name])
        if ("yin", name) not in _ref:   # the d' of the case, shared by every K
            _ref["yin", name] = R.reference(name) if name in R.cases() else R.yin(x, **kw)
        _ref[name, K] = candidates(x, K=K, yin=_ref["yin", name], **kw)
    return _ref[name, K]


def track_reference(name, K=7):
    """Float64 candidates and path (lag_ref = tau_min, default costs) of a case, computed once and shared."""
    if ("track", name, K) not in _ref:
        x, kw = (R.cases()[name] if name in R.cases() else e2e_cases()[name])
        c = cand_reference(name, K)
        _ref["track", name, K] = dict(c, **viterbi(c["period"], c["ap"], kw["sample_rate"], float(kw["tau_min"]), **COSTS))
    return _ref["track", name, K]


# ---- random candidate tensors for the path kernel alone -------------------------------------------------------------------
PATH_SHAPES = [(F, K) for F in (1, 2, 63, 64, 65, 130) for K in (1, 2, 7)]
PATH_B = 5
LDS_FRAMES = 4096   # csrc/f0_viterbi.hip VIT_CH: the backpointers of longer utterances go through the workspace
PATH_SHAPES_SWITCH = [(LDS_FRAMES, 1), (LDS_FRAMES + 1, 1), (2 * LDS_FRAMES + 8, 1)]


def random_candidates(F, K, seed):
    """(period, ap) fp32 (5, F, K): slot k near k + 1 times a period of 40 .. 57 samples that differs by row (3 % jitter, so
    ascending), ap in 0 .. 0.6 around the unvoiced cost, absent slots sprinkled in, frames with every slot absent, row 3
    entirely absent, rows 1 and 2 with absent first and last frames, and some ap of NaN and of +inf on slots whose period
    is positive."""
    rng = np.random.default_rng(seed)
    B = PATH_B
    base = rng.uniform(40.0, 57.0, (B, 1, 1))
    period = base * np.arange(1, K + 1) * (1 + 0.03 * rng.normal(0, 1, (B, F, K)))
    ap = rng.uniform(0.0, 0.6, (B, F, K))
    gone = rng.random((B, F, K)) < 0.2
    gone |= (rng.random((B, F)) < 0.1)[..., None]
    gone[3] = True
    gone[1, 0], gone[1, -1], gone[2, -1] = True, True, True
    period[gone], ap[gone] = 0.0, np.inf
    odd = (rng.random((B, F, K)) < 0.05) & ~gone
    ap[odd] = np.where(rng.random(int(odd.sum())) < 0.5, np.nan, np.inf)
    return period.astype(np.float32), ap.astype(np.float32)


def path_seed(F, K):
    """The seed of the random candidates of a shape: the first from 0 on whose float64 path has margin >= 1e-6 (asserted
    by the host test for every shape)."""
    if (F, K) not in _cache:
        for seed in range(100):
            p, a = random_candidates(F, K, seed)
            ref = viterbi(p, a, 24000.0, 24.0, **COSTS)
            if ref["margin"] >= 1e-6:
                _cache[F, K] = (seed, p, a, ref)
                break
    return _cache[F, K]
