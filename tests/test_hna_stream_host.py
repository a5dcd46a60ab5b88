"""CPU: the host side of the block-by-block harmonic-plus-noise analysis (analysis_stream.HarmonicNoiseStream,
functional.harmonic_analysis_stream, golf_harmonic_analysis_stream_f32) -- the finality and buffer rules against a brute-force
statement of them, the stream's bookkeeping driven with the float64 restatement (tests/hna_ref.py) indexed as the new entry
defines, and every refusal that needs no device (none launches)."""
import numpy as np
import pytest
import torch

import hna_ref as R

from golf_amd import analysis_stream as AS
from golf_amd import functional as GF
from golf_amd._lib import GolfError
from golf_amd.audiotensor import AudioTensor
from golf_amd.hna import HarmonicNoiseAnalysis


# ---- geometry ------------------------------------------------------------------------------------------------------------
def brute_final(pushed, f0_received, span, hop):
    """Frames from 0 on for which every one of the ``span`` samples of the longest window has come (a sample below 0 always
    has) and so has the next f0 frame."""
    f = 0
    while True:
        window = range(f * hop - span // 2, f * hop - span // 2 + span)
        if not (all(t < pushed for t in window) and f + 1 < f0_received):
            return f
        f += 1


GEOMETRY = [(1, 8), (1, 9), (16, 64), (16, 33), (240, 2048), (240, 961), (100, 48), (50, 7)]   # (hop, Lmax); the last two: hop > Lmax


@pytest.mark.parametrize("hop,span", GEOMETRY)
def test_finality_against_brute_force(hop, span):
    rng = np.random.default_rng(hop * 1000 + span)
    for order in ("audio ahead", "f0 ahead", "mixed"):
        pushed = got = 0
        emitted = 0
        for _ in range(40):
            n = int(rng.choice([0, 0, 1, hop - 1, hop, hop + 1, span, 3 * span + 1]))
            k = int(rng.choice([0, 0, 1, 2, 5]))
            if order == "audio ahead":
                n, k = 2 * n, (k if pushed > 6 * span else 0)
            elif order == "f0 ahead":
                n, k = (n if got > 12 else 0), k + 1
            pushed, got = pushed + n, got + k
            final = AS.hna_frames_final(pushed, got, span, hop)
            assert final == brute_final(pushed, got, span, hop), (order, pushed, got)
            assert final >= emitted   # monotone: a frame that was final stays final
            emitted = final
        assert emitted > 0, order


@pytest.mark.parametrize("hop,span", GEOMETRY)
def test_buffers_keep_what_an_open_frame_can_read(hop, span):
    for nxt in (0, 1, 2, 3, 17, 1000):
        x_from, f_from = AS.hna_keep_from(nxt, span, hop)
        reads = [t for f in range(nxt, nxt + 3) for t in range(f * hop - span // 2, f * hop - span // 2 + span) if t >= 0]
        assert x_from == min(reads)
        assert f_from == min(g for f in range(nxt, nxt + 3) for g in (f - 1, f, f + 1) if g >= 0)


@pytest.mark.parametrize("hop,span", GEOMETRY)
def test_latency_is_the_smallest_lag(hop, span):
    m = HarmonicNoiseAnalysis(24000, hop, 4, max_window=span, unvoiced_window=max(span // 2, 2), min_window=1)
    st = AS.HarmonicNoiseStream(m, 2)
    assert st.span == span
    for f in (0, 1, 5, 40):
        lag = next(d for d in range(0, span + hop + 2) if brute_final(f * hop + d, 10 ** 6, span, hop) > f)
        assert lag == st.latency == AS.frame_reach(span, True)
    # the unvoiced window may be the longer one
    m = HarmonicNoiseAnalysis(24000, hop, 4, max_window=max(span // 2, 2), unvoiced_window=span, min_window=1)
    assert AS.HarmonicNoiseStream(m, 1).latency == span - span // 2


def test_latency_at_the_defaults():
    st = AS.open_analysis_stream(HarmonicNoiseAnalysis(24000, 240, 155, n_mag=256), 2)
    assert type(st) is AS.HarmonicNoiseStream and st.latency == 1024 and st.hop == 240
    from golf_amd.f0 import F0Tracker

    f0_st = AS.F0TrackerStream(F0Tracker(24000, 240), 2, lag=8)
    assert f0_st.latency == 2520 and max(st.latency, st.hop + f0_st.latency) == 2760


# ---- the bookkeeping, driven with the float64 restatement ------------------------------------------------------------------
class HostStream(AS.HarmonicNoiseStream):
    """The stream with the device left out: ``_take`` makes every check and then accepts the CPU tensor, and ``_frames`` is
    tests/hna_ref.py on the buffers, laid out in the utterance as golf_harmonic_analysis_stream_f32 defines: samples
    ``[x_t0, x_t0 + n_x)``, f0 frames ``[f0_first, f0_first + n_f0)``, the neighbour rules of the entry.  What lies before the
    buffers is poisoned, so that a frame that reads it cannot come out right."""

    def __init__(self, module, batch_size):
        super().__init__(module, batch_size)
        self.calls = []

    def _device(self):
        return torch.device("cpu")

    def _take(self, t, name, hop):
        try:
            return super()._take(t, name, hop)
        except GolfError as e:
            assert "no CPU path" in str(e)
            return (t.as_tensor() if isinstance(t, AudioTensor) else t).detach()

    def _frames(self, x, f0, x_t0, f_first, f0_first, k, last, phases):
        with pytest.raises(GolfError, match="no CPU path"):   # the wrapper's own preconditions hold: only the device is missing
            super()._frames(x, f0, x_t0, f_first, f0_first, k, last, phases)
        self.calls.append((x_t0, x.shape[1], f_first, f0_first, f0.shape[1], k, last))
        assert (x_t0 + x.shape[1], f0_first + f0.shape[1]) == (self.pushed, self.f0_received)   # the buffers end at all that came
        m, B = self.module, self.B
        n_mag = m.n_mag or 0
        if k:
            xv = np.full((B, x_t0 + x.shape[1]), np.nan, np.float32)
            xv[:, x_t0:] = x.numpy()
            fv = np.full((B, f0_first + f0.shape[1]), 12345.0, np.float32)
            fv[:, f0_first:] = f0.numpy()
            # the utterance as far as the entry knows it: its frames end with the f0 buffer, its samples with the x buffer.
            # Without ``last`` the precondition says no computed frame reads beyond either.
            with np.errstate(all="ignore"):
                ref = R.analyse(xv, fv, m.sample_rate, self.hop, m.num_harmonics, n_mag, m.periods, m.min_window, m.max_window,
                                m.unvoiced_window, m.smooth, m.eps)
            sl = slice(f_first, f_first + k)
            out = [ref["amp"][:, sl], ref["phase"][:, sl]] + ([ref["log_mag"][:, sl]] if n_mag else [])
        else:
            out = [np.zeros((B, 0, m.num_harmonics))] * 2 + ([np.zeros((B, 0, n_mag))] if n_mag else [])
        if not phases:
            del out[1]
        out = [torch.tensor(np.ascontiguousarray(a)) for a in out]
        return out[0] if len(out) == 1 else tuple(out)


def assert_exact_trimming(calls, keep_from):
    """Every recorded call ``(x_t0, n_x, f_first, f0_first, n_f0, k, last)`` starts its buffers where the call before it left
    them: at ``keep_from(next frame)`` or, where less had come, at what had come; at 0 in an utterance's first call."""
    prev = None   # (samples, f0 frames) received at the previous call of the same utterance
    for x_t0, n_x, f_first, f0_first, n_f0, k, last in calls:
        if prev is None:
            assert (x_t0, f0_first) == (0, 0)
        else:
            x_from, f_from = keep_from(f_first)
            assert (x_t0, f0_first) == (min(x_from, prev[0]), min(f_from, prev[1]))
        prev = None if last else (x_t0 + n_x, f0_first + n_f0)


def make_signal(B, T, F, f_lo, f_hi, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 0.3, (B, T)).astype(np.float32)
    f0 = rng.uniform(f_lo, f_hi, (B, F)).astype(np.float32)
    f0[rng.uniform(size=(B, F)) < 0.3] = 0          # unvoiced gaps: every chirp rule occurs
    f0[0, :2] = [f_lo, 0.0]
    f0[-1, -2:] = [0.0, f_hi]
    return x, f0


def random_cuts(n, sizes, rng):
    cuts = []
    while sum(cuts) < n:
        cuts.append(min(int(rng.choice(sizes)), n - sum(cuts)))
    return cuts


def drive(st, x, f0, rng, x_sizes, f_sizes, mode="mixed"):
    """Push x and f0 in random cuts, interleaved at random; the concatenation of everything that came out, and the frames per
    call."""
    xc, fc = random_cuts(x.shape[1], x_sizes, rng), random_cuts(f0.shape[1], f_sizes, rng)
    xt, ft = torch.tensor(x), torch.tensor(f0)
    if mode == "f0 first":
        events = [("f", n) for n in fc] + [("x", n) for n in xc]
    elif mode == "audio first":
        events = [("x", n) for n in xc] + [("f", n) for n in fc]
    else:
        events = [("x", n) for n in xc] + [("f", n) for n in fc] + [("b", 0)] * 3
        order = rng.permutation(len(events))
        # a permutation keeps each input's own order: the cuts are taken from a running position
        events = [events[i] for i in order]
    px = pf = 0
    outs, counts = [], []
    for kind, n in events:
        if kind == "x":
            o = st.push_all(x=xt[:, px:px + n])
            px = min(px + n, x.shape[1])   # the "both" events took samples of their own: the last cuts come out shorter
        elif kind == "f":
            o = st.push_all(f0=AudioTensor(ft[:, pf:pf + n], st.hop))
            pf = min(pf + n, f0.shape[1])
        else:   # both at once, a sample and a frame if any is left
            o = st.push_all(AudioTensor(xt[:, px:px + 1]), ft[:, pf:pf + 1])
            px, pf = min(px + 1, x.shape[1]), min(pf + 1, f0.shape[1])
        outs.append(o)
        counts.append(o[0].shape[1])
    assert px == x.shape[1] and pf == f0.shape[1]
    outs.append(st.finish_all())
    counts.append(outs[-1][0].shape[1])
    return [torch.cat([o[i] for o in outs], 1).numpy() for i in range(len(outs[0]))], counts


# name -> (module arguments, T, F, f0 range): hop 1 with an odd Lmax, hop 16, and a hop above Lmax
HOST_CASES = {
    "hop1": (dict(sample_rate=24000.0, hop_length=1, num_harmonics=3, n_mag=5, min_window=2, max_window=17, unvoiced_window=12,
                  smooth=1), 37, 41, (6000.0, 11000.0)),
    "hop16": (dict(sample_rate=24000.0, hop_length=16, num_harmonics=3, n_mag=5, min_window=32, max_window=48,
                   unvoiced_window=64), 290, 20, (1500.0, 3000.0)),
    "hop80": (dict(sample_rate=24000.0, hop_length=80, num_harmonics=2, n_mag=None, min_window=8, max_window=33,
                   unvoiced_window=20), 900, 11, (3000.0, 6000.0)),
}


@pytest.mark.parametrize("name", list(HOST_CASES))
@pytest.mark.parametrize("mode", ["mixed", "f0 first", "audio first"])
def test_offset_indexing_against_the_float64_restatement(name, mode):
    kw, T, F, (lo, hi) = HOST_CASES[name]
    m = HarmonicNoiseAnalysis(**kw)
    hop, span = kw["hop_length"], max(kw["max_window"], kw["unvoiced_window"])
    x, f0 = make_signal(2, T, F, lo, hi, seed=len(name))
    ref = R.analyse(x, f0, kw["sample_rate"], hop, kw["num_harmonics"], kw["n_mag"] or 0, 4, kw["min_window"],
                    kw["max_window"], kw["unvoiced_window"], kw.get("smooth", 0))
    assert {"central", "forward", "backward", "none", "unvoiced"} <= set(ref["rule"].ravel()) or name == "hop80"
    want = [ref["amp"], ref["phase"]] + ([ref["log_mag"]] if kw["n_mag"] else [])
    st = HostStream(m, 2)
    for seed in (1, 2):   # the second utterance runs on the same stream, after finish()
        rng = np.random.default_rng(seed)
        got, counts = drive(st, x, f0, rng, [0, 1, 2, hop, span + 3, 2 * span + 1], [0, 1, 1, 2, 5], mode)
        assert sum(counts) == F and len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        assert (st.pushed, st.f0_received, st.framed) == (0, 0, 0)
    assert_exact_trimming(st.calls, lambda nxt: AS.hna_keep_from(nxt, span, hop))
    launches = [c for c in st.calls if c[5]]
    assert len(launches) >= 3 or mode != "mixed"
    # something was dropped on the way: a later call starts above sample 0 and above frame 0
    assert any(c[0] > 0 for c in launches) and any(c[3] > 0 for c in launches)
    # and no buffer is longer than what the lagging input explains: with the inputs in step it stays within a few windows
    if mode == "mixed" and name != "hop1":
        assert max(c[1] for c in st.calls) < T


def test_forward_types_and_counts_at_finish():
    """push / finish return what forward returns; finish() emits one frame per f0 frame for T far below, equal to and far
    above (F - 1) hop, equal to the restatement on the same (x, f0)."""
    kw, _, F, (lo, hi) = HOST_CASES["hop16"]
    m = HarmonicNoiseAnalysis(**kw)
    for T in (0, 5, (F - 1) * 16, (F - 1) * 16 + 1, (F - 1) * 16 + 1000):
        x, f0 = make_signal(2, T, F, lo, hi, seed=T)
        ref = R.analyse(x, f0, kw["sample_rate"], 16, 3, 5, 4, 32, 48, 64)
        st = HostStream(m, 2)
        first = st.push(torch.tensor(x), torch.tensor(f0))
        rest = st.finish()
        for pair in (first, rest):
            assert len(pair) == 2 and all(isinstance(t, AudioTensor) and t.hop_length == 16 for t in pair)
        n_first = AS.hna_frames_final(T, F, 64, 16)
        assert first[0].shape == (2, n_first, 3) and first[1].shape == (2, n_first, 5)
        assert rest[0].shape == (2, F - n_first, 3)
        assert np.array_equal(torch.cat([first[0].as_tensor(), rest[0].as_tensor()], 1).numpy(), ref["amp"])
        assert np.array_equal(torch.cat([first[1].as_tensor(), rest[1].as_tensor()], 1).numpy(), ref["log_mag"])
    # no f0 frame at all: empty results, whatever audio came
    st = HostStream(m, 2)
    st.push(x=torch.zeros(2, 500))
    out = st.finish_all()
    assert [tuple(t.shape) for t in out] == [(2, 0, 3), (2, 0, 3), (2, 0, 5)]
    # amplitudes alone when n_mag is None
    only = HostStream(HarmonicNoiseAnalysis(**HOST_CASES["hop80"][0]), 1)
    a = only.push(torch.zeros(1, 200), torch.full((1, 3), 4000.0))
    assert isinstance(a, AudioTensor) and a.shape == (1, 2, 2)
    assert only.finish().shape == (1, 1, 2)


# ---- refusals without a device -----------------------------------------------------------------------------------------------
def test_functional_refuses_before_a_launch():
    assert "harmonic_analysis_stream" in GF.__all__ and "harmonic_analysis" in GF.__all__
    x, f0 = torch.zeros(2, 3000), torch.full((2, 12), 100.0)
    base = dict(x_t0=0, f_first=0, f0_first=0, n_frames=8, last=False, sample_rate=24000, hop=240, num_harmonics=20)

    def call(x=x, f0=f0, **kw):
        return GF.harmonic_analysis_stream(x, f0, **dict(base, **kw))

    with pytest.raises(GolfError, match="no CPU path"):   # everything holds: only the device is missing
        call()
    with pytest.raises(GolfError, match="no CPU path"):
        call(n_frames=0)
    with pytest.raises(GolfError, match="no CPU path"):
        call(x=x[:0], f0=f0[:0])
    with pytest.raises(GolfError, match="must be \\(B, T\\)"):
        call(x=torch.zeros(3000))
    with pytest.raises(GolfError, match="f0 must be \\(B, F\\)"):
        call(f0=f0[:1])
    for kw, what in ((dict(hop=0), "hop"), (dict(num_harmonics=257), "num_harmonics"), (dict(n_mag=1), "n_mag"),
                     (dict(n_mag=514), "n_mag"), (dict(periods=1), "periods"), (dict(max_window=4096), "max_window"),
                     (dict(min_window=4096), "min_window"), (dict(unvoiced_window=4096), "unvoiced_window"),
                     (dict(n_mag=65, smooth=65), "smooth"), (dict(sample_rate=0), "sample_rate"), (dict(eps=-1), "eps"),
                     (dict(n_frames=-1), "n_frames"), (dict(x_t0=-1), "x_t0"), (dict(f0_first=-1), "f0_first"),
                     (dict(f_first=-1), "f_first"), (dict(f_first=2 ** 61), "f_first"),
                     # Lmax = 2048: frame 5 may start at sample 176 and frame 8 may end at 2944; frame 4 precedes frame 5
                     (dict(f_first=5, n_frames=4, x_t0=177), "x_t0"), (dict(f_first=5, n_frames=4, f0_first=5), "f0_first"),
                     (dict(f_first=0, f0_first=1), "f0_first"), (dict(n_frames=13, last=True), "n_f0"),
                     (dict(n_frames=10), "n_x"), (dict(f_first=5, n_frames=7, x_t0=176, x=torch.zeros(2, 5000)), "n_f0"),
                     (dict(f_first=5, n_frames=4, x_t0=176, x=x[:, :2767]), "n_x")):
        with pytest.raises(GolfError, match=what):
            call(**kw)
    # the same windows are accepted at their limits
    for kw in (dict(f_first=5, n_frames=4, x_t0=176, f0_first=4, x=x[:, :2768], f0=f0[:, :6]),
               dict(f_first=5, n_frames=7, x_t0=176, f0_first=4, x=x[:, :1], f0=f0[:, :8], last=True),
               dict(n_frames=12, last=True, x=x[:, :0])):
        with pytest.raises(GolfError, match="no CPU path"):
            call(**kw)


def test_c_entry_refuses_before_a_launch():
    from golf_amd import _lib

    lib = _lib.load()
    assert "golf_harmonic_analysis_stream_f32" in _lib.SIGNATURES and lib.golf_abi_version() == 6
    EINVAL, fake = -1, 256   # the pointers are never dereferenced

    def call(x=fake, xs=None, x_t0=176, n_x=2768, f0=fake, fs=None, f0_first=4, n_f0=6, amp=fake, phases=fake, log_mag=fake,
             B=2, f_first=5, n_frames=4, last=0, K=20, n_mag=65, hop=240, periods=4, min_window=480, max_window=2048,
             unvoiced_window=960, smooth=0, sr=24000.0, eps=1e-12):
        rc = lib.golf_harmonic_analysis_stream_f32(x, n_x if xs is None else xs, x_t0, n_x, f0, n_f0 if fs is None else fs,
                                                   f0_first, n_f0, amp, phases, log_mag, B, f_first, n_frames, last, K,
                                                   n_mag, hop, periods, min_window, max_window, unvoiced_window, smooth, sr,
                                                   eps, None)
        if rc:
            assert b"harmonic_analysis_stream" in lib.golf_last_error()
        return rc

    for kw, word in ((dict(x=None), b"null"), (dict(f0=None), b"null"), (dict(amp=None), b"null"), (dict(B=0), b"size"),
                     (dict(n_x=-1), b"size"), (dict(n_f0=0), b"size"), (dict(n_frames=0), b"size"), (dict(xs=2767), b"stride"),
                     (dict(fs=5), b"stride"), (dict(K=0), b"harmonics"), (dict(K=257), b"harmonics"), (dict(n_mag=1), b"n_mag"),
                     (dict(n_mag=514), b"n_mag"), (dict(hop=0), b"hop"), (dict(periods=1), b"periods"),
                     (dict(min_window=2049), b"min_window"), (dict(max_window=2049), b"max_window"),
                     (dict(unvoiced_window=2049), b"unvoiced_window"), (dict(unvoiced_window=1), b"unvoiced_window"),
                     (dict(smooth=65), b"smooth"), (dict(sr=0.0), b"sample_rate"), (dict(eps=-1.0), b"eps"),
                     (dict(B=1 << 20, n_frames=1 << 11), b"2^31"), (dict(x_t0=-1), b"x_t0"), (dict(f0_first=-1), b"f0_first"),
                     (dict(f_first=-1), b"f_first"), (dict(f_first=1 << 61), b"f_first"),
                     # the preconditions of the position: each one step beyond its limit
                     (dict(x_t0=177, n_x=2767), b"x_t0"), (dict(f0_first=5, n_f0=5), b"f0_first"),
                     (dict(f_first=0, x_t0=0, f0_first=1), b"f0_first"), (dict(n_f0=4, last=1), b"n_f0"),
                     (dict(n_x=2767), b"n_x"), (dict(n_f0=5), b"n_f0"),
                     # the unvoiced window may be the longer one: Lmax = 2048 again
                     (dict(max_window=1024, unvoiced_window=2048, x_t0=177, n_x=2767), b"x_t0")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())
    call(n_x=2767)
    assert b"last is not set" in lib.golf_last_error()
    call(n_f0=5)
    assert b"last is not set" in lib.golf_last_error()


def test_stream_surface_without_a_device():
    from golf_amd.f0 import F0Analysis
    from golf_amd.lpc import LPCAnalysis

    assert {"HarmonicNoiseStream", "open_analysis_stream", "hna_frames_final", "hna_keep_from"} <= set(AS.__all__)
    assert {"F0Stream", "F0TrackerStream", "LPCAnalysisStream", "frames_open", "frames_final", "frame_reach"} <= set(AS.__all__)
    m = HarmonicNoiseAnalysis(24000, 240, 20, n_mag=65)
    assert type(AS.open_analysis_stream(m, 3)) is AS.HarmonicNoiseStream
    assert type(AS.open_analysis_stream(F0Analysis(24000, 240), 3)) is AS.F0Stream
    assert type(AS.open_analysis_stream(LPCAnalysis(22, 240), 3)) is AS.LPCAnalysisStream
    with pytest.raises(TypeError, match="no analysis stream"):
        AS.open_analysis_stream(torch.nn.Identity(), 3)
    with pytest.raises(TypeError, match="HarmonicNoiseAnalysis is needed"):
        AS.HarmonicNoiseStream(F0Analysis(24000, 240), 3)
    with pytest.raises(ValueError, match="batch_size"):
        AS.HarmonicNoiseStream(m, 0)
    st = AS.HarmonicNoiseStream(m, 3)
    x, f0 = torch.zeros(3, 100), torch.zeros(3, 2)
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(x=x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(f0=f0.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="B=3"):
        st.push(x=x[:2])
    with pytest.raises(ValueError, match="B=3"):
        st.push(f0=f0[:2])
    with pytest.raises(ValueError, match="B=3"):
        st.push(x=x[0])
    with pytest.raises(AssertionError, match="hop 1"):
        st.push(x=AudioTensor(x, 2))
    with pytest.raises(AssertionError, match="hop 240"):
        st.push(f0=AudioTensor(f0, 120))
    for kw in (dict(x=x), dict(f0=f0), dict(x=x, f0=f0), dict(x=x.double())):
        with pytest.raises(GolfError, match="no CPU path"):
            st.push(**kw)
    assert (st.pushed, st.f0_received, st.framed) == (0, 0, 0)   # a refused push leaves the stream as it was
