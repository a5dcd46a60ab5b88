"""CPU: the host side of the streaming analysis -- the float64 restatement of the fixed-lag path (tests/f0_stream_ref.py)
against the whole-utterance path, the per-frame argmin and brute force; the margin that makes the GPU test's state equality a
fair demand; what the lag buys on the end-to-end cases; the arithmetic of which frames a call writes; the geometry of the
frame-local streams; and the refusals of the C entry (none launches) and of the Python layer without a device."""
import math
import os
import re

import numpy as np
import pytest
import torch

import f0_stream_ref as SR
import f0_track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR_, REF = 24000.0, 24.0


# ---- the fixed-lag path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,K", [(1, 1), (2, 7), (5, 2), (65, 2), (130, 7)])
def test_a_lag_of_the_whole_utterance_is_the_one_shot_path(F, K):
    p, a = TR.random_candidates(F, K, 0)
    full = TR.viterbi(p, a, SR_, REF, **TR.COSTS)
    for lag in (max(F - 1, 0), F, F + 3, SR.MAX_LAG):
        got = SR.fixed_lag(p, a, lag, SR_, REF, **TR.COSTS)
        assert np.array_equal(got["state"], full["state"]) and np.array_equal(got["f0"], full["f0"])
        assert got["margin"] >= full["margin"]   # it consults fewer end states than it has predecessor choices in common


@pytest.mark.parametrize("F,K", [(1, 1), (5, 2), (64, 7)])
def test_lag_zero_is_the_argmin_of_every_frame(F, K):
    p, a = TR.random_candidates(F, K, 0)
    got = SR.fixed_lag(p, a, 0, SR_, REF, **TR.COSTS)
    for b in range(TR.PATH_B):
        for f in range(F):   # C[f, .] is the cost of the best path of the utterance cut after frame f
            assert got["state"][b, f] == TR.viterbi_row(p[b, :f + 1], a[b, :f + 1], SR_, REF, **TR.COSTS)[0][f]


@pytest.mark.parametrize("F,K", [(F, K) for F in (1, 2, 3, 5) for K in (1, 2)])
def test_tiny_utterances_against_every_path(F, K):
    """The definition by brute force: s(g | h) is frame g of the cheapest of all paths over frames 0 .. h."""
    checked = 0
    for seed in range(4):
        p, a = TR.random_candidates(F, K, 2000 + seed)
        for b in range(TR.PATH_B):
            for lag in range(F + 1):
                state, f0, margin = SR.fixed_lag_row(p[b], a[b], lag, SR_, REF, **TR.COSTS)
                assert ((f0 == 0) == (state == 0)).all()
                if margin <= 1e-9:
                    continue
                for g in range(F):
                    h = min(g + lag, F - 1)
                    best, paths = TR.brute_force(p[b, :h + 1], a[b, :h + 1], REF, **TR.COSTS)
                    assert len(paths) == 1 and paths[0][g] == state[g]
                    checked += 1
    assert checked >= 4 * F


# ---- the shapes of the GPU test and their margin ---------------------------------------------------------------------------
def test_shape_and_lag_lists():
    assert SR.PATH_SHAPES == [(F, K) for F in (1, 2, 63, 64, 65, 130) for K in (1, 7)] + [(400, 2)]
    assert SR.lags_of(400) == [0, 1, 2, 7, 63, 64, 65, 399, 400, 1024]
    assert SR.lags_of(1) == [0, 1, 2, 7, 63, 64, 65, 1024] and SR.lags_of(64) == [0, 1, 2, 7, 63, 64, 65, 1024]
    assert SR.MAX_LAG == 1024 and SR.DEFAULT_LAG == 8 and TR.PATH_B == 5


@pytest.mark.parametrize("F,K", SR.PATH_SHAPES)
def test_margin_of_the_random_candidates(F, K):
    seed, p, a, refs = SR.path_seed(F, K)
    worst = min(r["margin"] for r in refs.values())
    print(f"F = {F}, K = {K}: seed {seed}, margin {worst:.2e} over lags {list(refs)}")
    assert 0 <= seed <= 99 and list(refs) == SR.lags_of(F)
    assert worst >= 1e-6
    full = TR.viterbi(p, a, SR_, REF, **TR.COSTS)
    for lag, r in refs.items():
        if lag >= F - 1:
            assert np.array_equal(r["state"], full["state"])
        assert (r["state"][3] == 0).all()   # the row without a candidate


def test_the_lag_is_exercised():
    seed, p, a, refs = SR.path_seed(130, 7)
    full = TR.viterbi(p, a, SR_, REF, **TR.COSTS)["state"]
    diff = {lag: int((refs[lag]["state"] != full).sum()) for lag in (0, 1, 2, 7)}
    print(f"(130, 7) seed {seed}: states that differ from the full path by lag: {diff}")
    assert diff[0] > diff[1] > diff[2] > 0


# ---- what the lag buys on the end-to-end cases --------------------------------------------------------------------------------
def _e2e(name, lag):
    ref = TR.track_reference(name)
    kw = TR.e2e_cases()[name][1]
    got = SR.fixed_lag(ref["period"], ref["ap"], lag, kw["sample_rate"], float(kw["tau_min"]), **TR.COSTS)
    return ref, got, TR.gross_errors(got["f0"], TR.truth(name))


@pytest.mark.parametrize("name", list(TR.e2e_cases()))
def test_end_to_end_cases_at_the_default_lag_and_at_lag_2(name):
    for lag in (SR.DEFAULT_LAG, 2):
        ref, got, errors = _e2e(name, lag)
        print(f"{name} lag {lag}: gross errors {errors}, margin {got['margin']:.2e}")
        assert np.array_equal(got["state"], ref["state"]) and (errors == 0).all()
        assert got["margin"] >= 1e-6


def test_lag_zero_has_gross_errors_on_the_noisy_rows():
    differs = []
    for name in TR.e2e_cases():
        ref, got, errors = _e2e(name, 0)
        differs.append(not np.array_equal(got["state"], ref["state"]))
        print(f"{name} lag 0: gross errors {errors}, {int((got['state'] != ref['state']).sum())} states differ")
        if name == "noisy":
            assert errors.sum() > 0
    assert all(differs)


# ---- which frames a call writes -----------------------------------------------------------------------------------------------
def test_decided_arithmetic_and_the_chunked_driver():
    from golf_amd import functional as GF

    for lag in (0, 1, 7, 64, 1024):
        for n in (0, 1, lag, lag + 1, 3 * lag + 2):
            assert SR.decided(n, lag) == GF.f0_viterbi_stream_decided(n, lag) == max(n - lag, 0)
            assert SR.decided(n, lag, True) == GF.f0_viterbi_stream_decided(n, lag, True) == n
    assert SR.calls([3, 0, 4, 2], 2) == [(0, 3, False, 0, 1), (3, 0, False, 1, 0), (3, 4, False, 1, 4), (7, 2, True, 5, 4)]
    assert SR.calls([9], 4, flush_alone=True) == [(0, 9, False, 0, 5), (9, 0, True, 5, 4)]
    assert SR.calls([2], 4, flush_alone=True) == [(0, 2, False, 0, 0), (2, 0, True, 0, 2)]
    # any implementation of the definition, replayed through any cuts, gives the uncut result: here the restatement itself,
    # run on the frames consumed so far
    for F, K in ((1, 1), (65, 2), (130, 7)):
        p, a = TR.random_candidates(F, K, 0)
        for lag in (0, 2, 7, 64, F):
            want = SR.fixed_lag(p, a, lag, SR_, REF, **TR.COSTS)

            def call(f_done, nf, flush, n_out):
                n = f_done + nf
                seen = SR.fixed_lag(p[:, :n], a[:, :n], lag, SR_, REF, **TR.COSTS)   # final in [0, decided(n, flush))
                hi = SR.decided(n, lag, flush)
                return seen["f0"][:, hi - n_out:hi], seen["state"][:, hi - n_out:hi]

            for name, (cuts, alone) in SR.cut_lists(F, lag).items():
                assert sum(cuts) == F and all(c >= 0 for c in cuts)
                f0, state = SR.run_cuts(call, F, cuts, lag, alone)
                assert np.array_equal(state, want["state"]) and np.array_equal(f0, want["f0"]), (F, K, lag, name)
    cuts = SR.cut_lists(130, 64)
    assert max(cuts["short"][0]) < 64 and 0 in cuts["random"][0] and cuts["alone"][1]


# ---- geometry of the frame-local streams ------------------------------------------------------------------------------------
GEOM = [(span, hop) for span in (1, 2, 5, 8, 51) for hop in (1, 3, 5, 8, 9, 60)]


@pytest.mark.parametrize("centred", (True, False))
def test_frame_geometry(centred):
    from golf_amd import functional as GF
    from golf_amd.analysis_stream import frame_reach, frames_final, frames_open

    for span, hop in GEOM:
        origin = -(span // 2) if centred else 0
        reach = frame_reach(span, centred)
        assert reach == origin + span
        prev = 0
        for n in range(3 * span + 2 * hop + 2):
            k = frames_open(n, span, hop, centred)
            assert k >= prev and k <= frames_final(n, span, hop, centred)        # monotone, never beyond the final count
            assert all(origin + f * hop + span <= n for f in range(k))            # every open frame lies below n
            assert origin + k * hop + span - 1 >= n                               # maximal: the next one reads sample >= n
            # latency is a bound (frame f is open once f * hop + reach samples have come) and is attained (not one sooner)
            for f in range(k + 2):
                assert (f < k) == (n >= f * hop + reach)
            prev = k
        for T in range(3 * span + 1):
            assert frames_final(T, span, hop, centred) == GF.f0_frames(T, span, hop, centred) \
                == GF.lpc_analysis_frames(T, span, hop, centred)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "f0_viterbi_stream.hip" in _lib.SOURCES
    assert lib.golf_abi_version() == _lib.ABI_VERSION == 6
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "golf_amd.h")).read(), flags=re.S)
    for name in ("golf_f0_viterbi_stream_state_bytes", "golf_f0_viterbi_stream_f32"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SIGNATURES
    EINVAL, EUNSUPPORTED = -1, -3
    fake = 256   # never dereferenced
    size = lib.golf_f0_viterbi_stream_state_bytes
    assert size(5, 7, 0) > 0 and size(5, 1, 1024) > size(5, 1, 1023) > 0 and size(1, 7, 8) * 5 == size(5, 7, 8)
    assert size(5, 7, 1024) >= 5 * (8 * 8 + 1024 * 8 + 1024 * 7 * 4)   # costs, backpointers and periods of 1024 frames
    assert size(0, 7, 8) == size(5, 0, 8) == size(5, 8, 8) == size(5, 7, -1) == size(5, 7, 1025) == 0

    def run(period=fake, ap=fake, f0=fake, state=fake, stride=None, carry=fake, carry_bytes=None, B=2, nf=5, K=7, lag=8,
            f_done=0, flush=0, sr=24000.0, lag_ref=24.0):
        n_out = SR.decided(f_done + nf, lag, flush) - SR.decided(f_done, lag)
        return lib.golf_f0_viterbi_stream_f32(period, ap, f0, state, max(n_out, 1) if stride is None else stride, carry,
                                              size(B, K, lag) if carry_bytes is None else carry_bytes, B, nf, K, lag, f_done,
                                              flush, sr, lag_ref, 0.3, 0.02, 0.35, 0.14, None)

    err = lib.golf_last_error
    assert run(lag=-1) == EUNSUPPORTED and b"f0_viterbi_stream" in err() and b"lag" in err()
    assert run(lag=1025) == EUNSUPPORTED and b"0..1024" in err()
    assert run(K=0) == EUNSUPPORTED and run(K=8) == EUNSUPPORTED and b"1..7" in err()
    assert run(nf=-1) == EINVAL and run(B=0) == EINVAL and run(f_done=-1) == EINVAL and b"bad size" in err()
    assert run(nf=0) == EINVAL and b"without flush" in err()
    assert run(nf=0, flush=1) == EINVAL and b"no frames" in err()
    assert run(period=None) == EINVAL and run(ap=None) == EINVAL and b"null" in err()
    assert run(carry=None) == EINVAL and b"carry" in err()
    assert run(carry_bytes=size(2, 7, 8) - 1) == EINVAL and b"carry" in err()
    assert run(carry=fake + 4) == EINVAL and b"aligned" in err()
    assert run(nf=20, f0=None, state=None) == EINVAL and b"at least one output" in err()
    assert run(nf=20, stride=11) == EINVAL and b"out_stride" in err()              # 12 frames written
    assert run(nf=5, flush=1, stride=4) == EINVAL and run(nf=0, f_done=30, flush=1, stride=7) == EINVAL
    assert run(f_done=2 ** 31 - 5) == EUNSUPPORTED and b"2^31" in err()
    assert run(B=1 << 16, nf=1 << 15, carry_bytes=1 << 40) == EUNSUPPORTED and b"2^31" in err()
    assert run(sr=0.0) == EINVAL and run(lag_ref=0.0) == EINVAL and run(sr=math.nan) == EINVAL and b"positive" in err()


def test_functional_and_streams_without_a_device():
    from golf_amd import analysis_stream as AS
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from golf_amd.f0 import F0Analysis, F0Tracker
    from golf_amd.lpc import LPCAnalysis

    assert {"f0_viterbi_stream", "f0_viterbi_stream_state"} <= set(GF.__all__)
    assert {"F0Stream", "F0TrackerStream", "LPCAnalysisStream", "open_analysis_stream"} <= set(AS.__all__)
    for B, K, lag, what in ((0, 7, 8, "rows"), (2, 0, 8, "1..7"), (2, 8, 8, "1..7"), (2, 7, -1, "lag"), (2, 7, 1025, "lag")):
        with pytest.raises(GolfError, match=what):
            GF.f0_viterbi_stream_state(B, K, lag, "cpu")
    carry = GF.f0_viterbi_stream_state(2, 3, 8, "cpu")
    assert carry.dtype == torch.int64 and carry.numel() * 8 == 2 * (192 + 40 * 8)
    p, a = torch.ones(2, 5, 3), torch.zeros(2, 5, 3)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.f0_viterbi_stream(p, a, carry, 0, 8, SR_, REF)
    for args, kw, what in (((p[0], a[0], carry, 0, 8, SR_, REF), {}, "B, F, K"), ((p, a[:, :, :2], carry, 0, 8, SR_, REF), {}, "B, F, K"),
                           ((torch.ones(2, 5, 8), torch.ones(2, 5, 8), carry, 0, 8, SR_, REF), {}, "1..7"),
                           ((p, a, carry, 0, 1025, SR_, REF), {}, "lag"), ((p, a, carry, -1, 8, SR_, REF), {}, "f_done"),
                           ((p[:, :0], a[:, :0], carry, 0, 8, SR_, REF), dict(flush=True), "no frames"),
                           ((p, a, carry, 0, 8, 0.0, REF), {}, "positive"), ((p, a, carry, 0, 8, SR_, 0.0), {}, "positive"),
                           ((p, a, carry, 2 ** 31 - 3, 8, SR_, REF), {}, "2\\^31")):
        with pytest.raises(GolfError, match=what):
            GF.f0_viterbi_stream(*args, **kw)

    yin, tracker, lpc = F0Analysis(24000, 240), F0Tracker(24000, 240), LPCAnalysis(8, 60)
    streams = [AS.open_analysis_stream(yin, 2), AS.open_analysis_stream(tracker, 2), AS.open_analysis_stream(lpc, 2)]
    assert [type(s) for s in streams] == [AS.F0Stream, AS.F0TrackerStream, AS.LPCAnalysisStream]
    assert streams[1].lag == 8 and AS.open_analysis_stream(tracker, 2, lag=3).lag == 3
    assert "not tuned on speech" in AS.F0TrackerStream.__doc__
    S = yin.window_length + yin.tau_max
    assert streams[0].latency == S - S // 2 and streams[1].latency == S - S // 2 + 8 * 240 and streams[2].latency == 120
    assert AS.F0Stream(F0Analysis(24000, 240, centred=False), 1).latency == S
    with pytest.raises(TypeError):
        AS.open_analysis_stream(torch.nn.Identity(), 2)
    with pytest.raises(TypeError, match="F0Tracker"):
        AS.F0TrackerStream(yin, 2)
    with pytest.raises(GolfError, match="lag"):
        AS.F0TrackerStream(tracker, 2, lag=1025)
    for s in streams:
        with pytest.raises(ValueError, match="batch_size"):
            type(s)(s.module, 0)
        with pytest.raises(GolfError, match="no CPU path"):
            s.push(torch.zeros(2, 100))
        with pytest.raises(ValueError, match="B=2"):
            s.push(torch.zeros(3, 100))
        with pytest.raises(NotImplementedError, match="requires grad"):
            s.push(torch.zeros(2, 100, requires_grad=True))


# ---- the sample buffer of the frame-local streams, with a frame-local stand-in for the kernels -------------------------------
WEIGHTS = [3, -1, 4, 1, -5, 9, 2, -6, 5]   # fixed integers: with small integers in x every sum is exact in fp32


def local_frames(x, k, span, hop):
    """``out[b, f] = sum_j WEIGHTS[j] x[b, f * hop + j]`` over ``j < span`` for the first k frames of x, which is zero beyond
    its end: what a one-shot kernel does with ``centred=False, n_frames=k``, frame by frame."""
    need = (k - 1) * hop + span
    x = torch.nn.functional.pad(x, (0, max(need - x.shape[1], 0)))[:, :need]
    return (x.unfold(1, span, hop) * torch.tensor(WEIGHTS[:span], dtype=x.dtype)).sum(-1)


def _host_frames(base):
    """``base`` with the device left out: ``_take`` makes every check and then accepts the CPU tensor, and ``_frames`` is the
    stand-in, shaped as the stream's own kernel shapes its results (``_shape``)."""
    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor

    class Host(base):
        block = 0   # the length of the block being pushed: the driver sets it

        def _device(self):
            return torch.device("cpu")

        def _take(self, t, *args):
            try:
                return super()._take(t, *args)
            except GolfError as e:
                assert "no CPU path" in str(e)
                return (t.as_tensor() if isinstance(t, AudioTensor) else t).detach()

        def _frames(self, x, k):
            assert k >= 1 and 1 <= x.shape[1] <= self.span + (k - 1) * self.hop + self.block   # nothing older is kept
            self.calls = getattr(self, "calls", 0) + 1
            return self._shape(local_frames(x, k, self.span, self.hop))

    return Host


def _frame_stream_classes():
    from types import SimpleNamespace

    from golf_amd import analysis_stream as AS
    from golf_amd.f0 import F0Analysis
    from golf_amd.lpc import LPCAnalysis

    class Plain(_host_frames(AS._FrameStream)):
        """The shared base alone: one (B, k) result."""

        def __init__(self, span, hop, centred, B):
            super().__init__(SimpleNamespace(hop_length=hop, centred=centred), B, span)

        def _shape(self, out):
            return (out,)

        def _emit(self, k, out, final):
            return out if k > 0 else (torch.empty(self.B, 0),)

        def push_all(self, x):
            return self._run(x, False)

        def finish_all(self):
            return self._run(None, True)

    class LPC(_host_frames(AS.LPCAnalysisStream)):
        def __init__(self, span, hop, centred, B):
            super().__init__(LPCAnalysis(2, hop, window_length=span, centred=centred), B, return_rc=True)

        def _shape(self, out):
            return out, torch.stack([out + 1, out + 2], -1), torch.stack([out + 3, out + 4], -1)

    class F0(_host_frames(AS.F0Stream)):
        def __init__(self, span, hop, centred, B):   # tau_max = 2, so span = window_length + 2
            super().__init__(F0Analysis(4.0, hop, f0_min=2.0, f0_max=3.0, window_length=span - 2, centred=centred), B)

        def _shape(self, out):
            return out, out + 1, out + 2

    return Plain, LPC, F0


@pytest.mark.parametrize("centred", (True, False))
@pytest.mark.parametrize("span,hop", [(8, 3), (7, 7), (4, 9), (9, 1), (1, 1)])   # hop below, at and above the span
def test_frame_streams_on_the_host(span, hop, centred):
    """``_FrameStream``'s buffer -- the zero prefix before sample 0, the samples dropped between frames when hop > span, the
    frames that read only zeros after the end, the reset at ``finish()`` -- under the base alone, ``LPCAnalysisStream`` and
    ``F0Stream`` (whose frame of window_length + tau_max samples cannot be 1 long): two utterances per stream, every
    length, random cuts, ``torch.equal`` to the stand-in over the whole zero-padded utterance."""
    from golf_amd.analysis_stream import frame_reach, frames_final

    B, sizes = 2, [0, 1, hop - 1, hop, hop + 1, span, 3 * span + 1]
    for cls in _frame_stream_classes():
        if cls.__name__ == "F0" and span < 3:
            continue
        st = cls(span, hop, centred, B)
        assert (st.span, st.hop, st.centred, st.latency) == (span, hop, centred, frame_reach(span, centred))
        launches = 0
        for i, T in enumerate((0, 1, span - 1, span, 5 * hop + span + 1, 5 * hop + span + 1)):
            rng = np.random.default_rng(1000 * span + 10 * hop + i)
            x = torch.tensor(rng.integers(-8, 9, (B, T)).astype(np.float32))
            F = frames_final(T, span, hop, centred)
            want = st._shape(local_frames(torch.nn.functional.pad(x, (span // 2 if centred else 0, 0)), F, span, hop))
            cuts = []
            while sum(cuts) < T:
                cuts.append(min(int(rng.choice(sizes)), T - sum(cuts)))
            cuts += [0] * (i % 2)   # an empty block after the last sample, every other utterance
            outs, p = [], 0
            for n in cuts:
                st.block = n
                outs.append(st.push_all(x[:, p:p + n]))
                p += n
                assert st.pushed == p and st.framed == sum(o[0].shape[1] for o in outs) <= F
            st.block = 0
            outs.append(st.finish_all())
            assert (st.pushed, st.framed) == (0, 0) and len(outs[0]) == len(want)
            for j, w in enumerate(want):
                assert all(o[j].shape[2:] == w.shape[2:] and o[j].dtype == w.dtype for o in outs)   # k = 0 included
                assert torch.equal(torch.cat([o[j] for o in outs], 1), w), (cls.__name__, T, cuts, j)
            launches += len(cuts) + 1
        assert 6 <= st.calls <= launches
