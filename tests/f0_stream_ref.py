"""Float64 restatement of the fixed-lag f0 path search (golf_f0_viterbi_stream_f32, include/golf_amd.h), written from the
definition with plain loops on top of ``f0_track_ref``: the forward recursion with its backpointers, e(f) = argmin_s C[f, s],
and for every frame g the walk from e(h), h = min(g + lag, F - 1), down to g.  ``margin`` is the smallest gap between best
and second best over every predecessor choice, every per-frame end state that the definition consults (h >= lag) and the
final end state: above roundoff the fixed-lag path is unique, so a kernel that computes the same costs to 1e-12 must return
the same states, however its input was cut.

Also here: ``decided`` and ``calls``, the arithmetic that says which frames a call writes, and ``run_cuts``, the driver that
replays a list of cuts through any implementation of one call.  It is the checker of csrc/f0_viterbi_stream.hip."""
import math

import numpy as np

import f0_ref as R            # noqa: F401 -- the cases of the stream tests
import f0_track_ref as TR

MAX_LAG = 1024
DEFAULT_LAG = 8
LAGS = (0, 1, 2, 7, 63, 64, 65, "F-1", "F", 1024)
PATH_SHAPES = [(F, K) for F in (1, 2, 63, 64, 65, 130) for K in (1, 7)] + [(400, 2)]


def lags_of(F):
    """The lags of the shape list for an utterance of F frames, each once."""
    out = []
    for lag in LAGS:
        lag = {"F-1": F - 1, "F": F}.get(lag, lag)
        if lag not in out:
            out.append(lag)
    return out


def _best(values):
    """(best, argbest, second) of a list with None for absent entries: the smaller index wins a tie."""
    best, arg, second = math.inf, -1, math.inf
    for i, v in enumerate(values):
        if v is None:
            continue
        if v < best:
            best, arg, second = v, i, best
        elif v < second:
            second = v
    return best, arg, second


def forward_row(period, ap, lag_ref, unvoiced_cost=0.3, lag_cost=0.02, jump_cost=0.35, switch_cost=0.14):
    """(F, K) -> back (F, K + 1) int, end (F,) int with e(f), end_gap (F,) and the smallest predecessor gap."""
    period, ap = np.asarray(period, np.float64), np.asarray(ap, np.float64)
    F, K = period.shape
    back, end, end_gap = np.zeros((F, K + 1), int), np.zeros(F, int), np.zeros(F)
    pred_gap = math.inf
    C = None
    for f in range(F):
        loc = TR._local(period[f], ap[f], lag_ref, unvoiced_cost, lag_cost)
        if f == 0:
            C = list(loc)
        else:
            new = [None] * (K + 1)
            for j in range(K + 1):
                if loc[j] is None:
                    continue
                best, arg, second = _best([None if C[i] is None else
                                           C[i] + TR._trans(i, j, period[f - 1], period[f], jump_cost, switch_cost)
                                           for i in range(K + 1)])
                pred_gap = min(pred_gap, second - best)
                new[j], back[f, j] = loc[j] + best, arg
            C = new
        best, arg, second = _best(C)
        end[f], end_gap[f] = arg, second - best
    return back, end, end_gap, pred_gap


def fixed_lag_row(period, ap, lag, sample_rate, lag_ref, **costs):
    """period, ap (F, K) -> (state (F,), f0 (F,), margin) of one utterance at ``lag``."""
    period = np.asarray(period, np.float64)
    F = period.shape[0]
    back, end, end_gap, margin = forward_row(period, ap, lag_ref, **costs)
    state = np.zeros(F, int)
    for g in range(F):
        h = min(g + lag, F - 1)
        margin = min(margin, end_gap[h])
        s = end[h]
        for k in range(h, g, -1):
            s = back[k, s]
        state[g] = s
    f0 = np.array([sample_rate / period[f, s - 1] if s > 0 else 0.0 for f, s in enumerate(state)])
    return state, f0, margin


def fixed_lag(period, ap, lag, sample_rate, lag_ref, **costs):
    """(B, F, K) -> dict: state (B, F) int, f0 (B, F), margin (the smallest over the rows)."""
    rows = [fixed_lag_row(period[b], ap[b], lag, sample_rate, lag_ref, **costs) for b in range(len(period))]
    return dict(state=np.array([r[0] for r in rows]), f0=np.array([r[1] for r in rows]),
                margin=min([r[2] for r in rows], default=math.inf))


# ---- which frames a call writes -------------------------------------------------------------------------------------------
def decided(n, lag, flush=False):
    return n if flush else max(n - lag, 0)


def calls(cuts, lag, flush_alone=False):
    """A list of cuts (frames per call) -> the calls ``(f_done, nf, flush, first, n_out)``: the last cut flushes, or with
    ``flush_alone`` a call of no frames after it does.  ``first`` is the frame of the call's column 0."""
    out, f_done = [], 0
    for i, nf in enumerate(cuts):
        flush = i == len(cuts) - 1 and not flush_alone
        first = decided(f_done, lag)
        out.append((f_done, nf, flush, first, decided(f_done + nf, lag, flush) - first))
        f_done += nf
    if flush_alone:
        first = decided(f_done, lag)
        out.append((f_done, 0, True, first, f_done - first))
    return out


def run_cuts(call, F, cuts, lag, flush_alone=False):
    """Replays the cuts through ``call(f_done, nf, flush, n_out) -> (f0, state)`` arrays of (B, n_out) and concatenates what
    the calls wrote; asserts that the calls tile [0, F)."""
    assert sum(cuts) == F
    f0s, states, at = [], [], 0
    for f_done, nf, flush, first, n_out in calls(cuts, lag, flush_alone):
        assert first == at and n_out >= 0
        f0, state = call(f_done, nf, flush, n_out)
        assert f0.shape[-1] == state.shape[-1] == n_out
        f0s.append(f0), states.append(state)
        at += n_out
    assert at == F
    return np.concatenate(f0s, -1), np.concatenate(states, -1)


def cut_lists(F, lag, seed=0):
    """name -> (cuts, flush_alone): everything in one call, a frame per call, calls shorter than the lag (they write
    nothing until the lag is filled), a seeded random cut, and the last frames arriving in a flush without frames."""
    rng = np.random.default_rng(1000 * F + lag + seed)
    short = max(min(lag, F) // 2, 1)
    rand, left = [], F
    while left:
        n = int(min(rng.integers(0, 48), left)) if rng.random() < 0.8 else 0
        rand.append(n)
        left -= n
    assert rand[-1] > 0   # calls without frames lie inside the list: the last call flushes the frames it brings
    return {"one": ([F], False), "each": ([1] * F, False), "alone": ([F], True),
            "short": ([short] * (F // short) + ([F % short] if F % short else []), False), "random": (rand, False)}


# ---- the random candidates of a shape: one seed whose margin holds at every lag ---------------------------------------------
_cache = {}


def path_seed(F, K):
    """(seed, period, ap, {lag: reference}) of a shape: the first seed from 0 on whose float64 fixed-lag paths have margin
    >= 1e-6 at every lag of the list (asserted by the host test)."""
    if (F, K) not in _cache:
        for seed in range(100):
            p, a = TR.random_candidates(F, K, seed)
            refs = {lag: fixed_lag(p, a, lag, 24000.0, 24.0, **TR.COSTS) for lag in lags_of(F)}
            if min(r["margin"] for r in refs.values()) >= 1e-6:
                _cache[F, K] = (seed, p, a, refs)
                break
    return _cache[F, K]
