"""CPU: the host side of the block-by-block spectral-envelope, residual and glottal-source analyses
(analysis_stream.SpectralEnvelopeStream / ResidualStream / GlottalSourceStream, functional.spectral_envelope_stream /
ltv_residual / ltv_residual_stream, golf_spectral_envelope_stream_f32 / golf_ltv_residual_f32 / golf_ltv_residual_stream_f32)
-- the finality and buffer rules against brute-force statements of them, the streams' bookkeeping driven with the float64
restatements (tests/env_ref.py, tests/hna_ref.py + tests/glottal_ref.py, tests/residual_ref.py) indexed as the new entries
define, and every refusal that needs no device (none launches)."""
import numpy as np
import pytest
import torch

import env_ref
import glottal_ref
import hna_ref
import residual_ref

from golf_amd import analysis_stream as AS
from golf_amd import functional as GF
from golf_amd._lib import GolfError
from golf_amd.audiotensor import AudioTensor
from golf_amd.envelope import SpectralEnvelopeAnalysis
from golf_amd.glottal import GlottalSourceAnalysis


# ---- geometry ------------------------------------------------------------------------------------------------------------
def env_brute_final(pushed, f0_received, hwmax, hop):
    """Frames from 0 on for which every sample within hwmax of the centre has come (a sample below 0 always has) and so has
    the frame's own f0."""
    f = 0
    while all(t < pushed for t in range(f * hop - hwmax, f * hop + hwmax + 1)) and f < f0_received:
        f += 1
    return f


def res_brute_final(pushed, frames_received, hop):
    """Samples from 0 on that have come and whose next frame has come."""
    t = 0
    while t < pushed and t // hop + 1 < frames_received:
        t += 1
    return t


ENV_GEOMETRY = [(1, 4), (1, 0), (16, 32), (16, 7), (80, 255), (80, 120), (80, 3), (80, 39)]   # (hop, hwmax); 2 hwmax + 1 on both sides of hop


@pytest.mark.parametrize("hop,hwmax", ENV_GEOMETRY)
def test_env_finality_against_brute_force(hop, hwmax):
    rng = np.random.default_rng(hop * 1000 + hwmax)
    span = 2 * hwmax + 1
    for order in ("audio ahead", "f0 ahead", "mixed"):
        pushed = got = emitted = 0
        for _ in range(40):
            n = int(rng.choice([0, 0, 1, hop - 1, hop, hop + 1, span, 3 * span + 1]))
            k = int(rng.choice([0, 0, 1, 2, 5]))
            if order == "audio ahead":
                n, k = 2 * n, (k if pushed > 6 * span else 0)
            elif order == "f0 ahead":
                n, k = (n if got > 12 else 0), k + 1
            pushed, got = pushed + n, got + k
            final = AS.env_frames_final(pushed, got, hwmax, hop)
            assert final == env_brute_final(pushed, got, hwmax, hop), (order, pushed, got)
            assert final >= emitted
            emitted = final
        assert emitted > 0, order


@pytest.mark.parametrize("hop,hwmax", ENV_GEOMETRY)
def test_env_buffers_keep_what_an_open_frame_can_read(hop, hwmax):
    for nxt in (0, 1, 2, 3, 17, 1000):
        x_from, f_from = AS.env_keep_from(nxt, hwmax, hop)
        assert x_from == min(t for f in range(nxt, nxt + 3) for t in range(f * hop - hwmax, f * hop + hwmax + 1) if t >= 0)
        assert f_from == nxt


@pytest.mark.parametrize("hop", [1, 16, 80])
def test_residual_finality_against_brute_force(hop):
    rng = np.random.default_rng(hop)
    for order in ("audio ahead", "frames ahead", "mixed"):
        pushed = got = emitted = 0
        for _ in range(40):
            n = int(rng.choice([0, 0, 1, hop - 1, hop, hop + 1, 3 * hop + 1]))
            k = int(rng.choice([0, 0, 1, 2, 5]))
            if order == "audio ahead":
                n, k = 2 * n, (k if pushed > 6 * hop else 0)
            elif order == "frames ahead":
                n, k = (n if got > 12 else 0), k + 1
            pushed, got = pushed + n, got + k
            final = AS.res_samples_final(pushed, got, hop)
            assert final == res_brute_final(pushed, got, hop), (order, pushed, got)
            assert emitted <= final <= AS.res_samples_finish(pushed, got, hop)   # finish() never takes a sample back
            assert AS.res_samples_finish(pushed, got, hop) == residual_ref.length(pushed, got, hop)
            emitted = final
        assert emitted > 0, order


@pytest.mark.parametrize("hop", [1, 16, 80])
@pytest.mark.parametrize("M", [1, 22, 64])
def test_residual_buffers_keep_what_a_later_sample_can_read(hop, M):
    for frames in (0, 1, 2, 3, 9):
        for emitted in sorted({0, 1, M - 1, M, M + 1, hop, 3 * hop - 1, 3 * hop, (frames - 1) * hop}):
            if not 0 <= emitted <= AS.res_samples_final(10 ** 6, frames, hop):
                continue
            x_from, f_from = AS.res_keep_from(emitted, frames, M, hop)
            assert x_from == min(t - 1 - i for t in (emitted, emitted + 1) for i in range(M) if t - 1 - i >= 0) \
                if emitted > 0 else x_from == 0
            # the next sample reads frame emitted // hop if more frames come, and min(emitted // hop, F - 2) if none does
            reads = [emitted // hop] + ([max(min(emitted // hop, frames - 2), 0)] if frames else [])
            assert f_from == min(reads)


@pytest.mark.parametrize("hop,hwmax", ENV_GEOMETRY)
def test_env_latency_is_the_smallest_lag(hop, hwmax):
    sr = 24000.0
    m = SpectralEnvelopeAnalysis(sr, hop, 2048, f0_floor=1.5 * sr / (hwmax + 0.25) if hwmax else 1.5 * sr / 0.4,
                                 f0_ceil=1e9, unvoiced_f0=1e8)   # only hwmax is read here
    st = AS.SpectralEnvelopeStream(m, 2)
    assert st.hwmax == hwmax and st.span == 2 * hwmax + 1
    for f in (0, 1, 5, 40):
        lag = next(d for d in range(0, hwmax + hop + 3) if env_brute_final(f * hop + d, 10 ** 6, hwmax, hop) > f)
        assert lag == st.latency == hwmax + 1


@pytest.mark.parametrize("hop", [1, 16, 80])
@pytest.mark.parametrize("d", [0, 5, 40, 480])
def test_residual_latency_is_the_smallest_lag(hop, d):
    """Frames that arrive d samples after their own time: frame g has come once ``pushed >= g hop + d``.  The largest, over
    the samples, of the smallest lag after which a sample is final is ``hop + d``."""
    st = AS.ResidualStream(hop, 4, 1)

    def frames(n):
        return (n - d) // hop + 1 if n >= d else 0

    lags = [next(lag for lag in range(1, hop + d + 3) if res_brute_final(t + lag, frames(t + lag), hop) > t)
            for t in range(0, 3 * hop + 2)]
    assert max(lags) == st.latency + d == hop + d
    assert lags[hop] == hop + d   # a sample on a frame's own time waits for the whole next hop


def test_latency_at_the_recipe():
    from golf_amd.lpc import LPCAnalysis

    lpc = AS.LPCAnalysisStream(LPCAnalysis(22, 240), 2)   # centred, window 960: a frame comes 480 samples after its own time
    assert lpc.latency == 480
    assert AS.ResidualStream(240, 22, 2).latency + lpc.latency == 240 + 480
    env = AS.open_analysis_stream(SpectralEnvelopeAnalysis(24000, 240, filter_order=80), 2)
    assert type(env) is AS.SpectralEnvelopeStream and env.latency == 512 and env.hwmax == 511
    glo = AS.open_analysis_stream(GlottalSourceAnalysis(torch.randn(4, 64), 24000, 240), 2)
    assert type(glo) is AS.GlottalSourceStream and glo.latency == 1024 and glo.span == 2048 and glo.unvoiced_window == 960


# ---- the bookkeeping, driven with the float64 restatements -------------------------------------------------------------------
def random_cuts(n, sizes, rng):
    cuts = []
    while sum(cuts) < n:
        cuts.append(min(int(rng.choice(sizes)), n - sum(cuts)))
    return cuts


def drive(push, finish, audio, ctrl, rng, a_sizes, c_sizes, mode):
    """Push the audio (B, T) and the controls (a list of arrays cut alike along axis 1) in random cuts, interleaved at random;
    ``push(audio block or None, control blocks or None)`` and ``finish()`` return tuples of arrays.  The concatenation of
    everything that came out, and the counts per call."""
    T, F = audio.shape[1], ctrl[0].shape[1]
    ac, cc = random_cuts(T, a_sizes, rng), random_cuts(F, c_sizes, rng)
    if mode == "controls first":
        events = [("c", n) for n in cc] + [("a", n) for n in ac]
    elif mode == "audio first":
        events = [("a", n) for n in ac] + [("c", n) for n in cc]
    else:
        events = [("a", n) for n in ac] + [("c", n) for n in cc] + [("b", 0)] * 3
        events = [events[i] for i in rng.permutation(len(events))]   # the cuts are taken from a running position
    pa = pc = 0
    outs = []
    for kind, n in events:
        if kind == "a":
            outs.append(push(audio[:, pa:pa + n], None))
            pa = min(pa + n, T)
        elif kind == "c":
            outs.append(push(None, [c[:, pc:pc + n] for c in ctrl]))
            pc = min(pc + n, F)
        else:   # both at once, a sample and a frame if any is left
            outs.append(push(audio[:, pa:pa + 1], [c[:, pc:pc + 1] for c in ctrl]))
            pa, pc = min(pa + 1, T), min(pc + 1, F)
    assert pa == T and pc == F
    outs.append(finish())
    return [np.concatenate([o[i] for o in outs], 1) for i in range(len(outs[0]))], [o[0].shape[1] for o in outs]


def assert_exact_trimming(calls, keep_from):
    """Every recorded call ``(x_t0, n_x, first, c_first, n_c, last)`` -- ``first`` the first frame or sample it computes --
    starts its buffers where the call before it left them: at ``keep_from(first, controls received then)`` or, where less had
    come, at what had come; at 0 in an utterance's first call."""
    prev = None   # (samples, control frames) received at the previous call of the same utterance
    for x_t0, n_x, first, c_first, n_c, last in calls:
        if prev is None:
            assert (x_t0, c_first) == (0, 0)
        else:
            x_from, c_from = keep_from(first, prev[1])
            assert (x_t0, c_first) == (min(x_from, prev[0]), min(c_from, prev[1]))
        prev = None if last else (x_t0 + n_x, c_first + n_c)


def frame_calls(calls):
    return [(x_t0, n_x, f_first, f0_first, n_f0, last) for x_t0, n_x, f_first, f0_first, n_f0, k, last in calls]


def tensors(blocks):
    return None if blocks is None else [torch.tensor(np.ascontiguousarray(b)) for b in blocks]


class _HostTake:
    """``_take`` makes every check and then accepts the CPU tensor."""

    def _device(self):
        return torch.device("cpu")

    def _take(self, t, *args):
        try:
            return super()._take(t, *args)
        except GolfError as e:
            assert "no CPU path" in str(e)
            return (t.as_tensor() if isinstance(t, AudioTensor) else t).detach()


def laid_out(buf, first, fill):
    """The buffer at its place in the utterance; what lies before it is poisoned."""
    buf = buf.numpy()
    full = np.full((buf.shape[0], first + buf.shape[1]) + buf.shape[2:], fill, buf.dtype)
    full[:, first:] = buf
    return full


class HostEnvStream(_HostTake, AS.SpectralEnvelopeStream):
    """``_frames`` is tests/env_ref.py on the buffers laid out as golf_spectral_envelope_stream_f32 defines."""

    def __init__(self, module, batch_size):
        super().__init__(module, batch_size)
        self.calls = []

    def _frames(self, x, f0, x_t0, f_first, f0_first, k, last, full):
        with pytest.raises(GolfError, match="no CPU path"):   # the wrapper's own preconditions hold: only the device is missing
            super()._frames(x, f0, x_t0, f_first, f0_first, k, last, full)
        self.calls.append((x_t0, x.shape[1], f_first, f0_first, f0.shape[1], k, last))
        assert (x_t0 + x.shape[1], f0_first + f0.shape[1]) == (self.pushed, self.f0_received)   # the buffers end at all that came
        m, nb = self.module, self.module.n_fft // 2 + 1
        n_ceps = nb if m.filter_order is None else m.filter_order + 1
        if k:
            xv, fv = laid_out(x, x_t0, np.nan), laid_out(f0, f0_first, np.nan)
            # the utterance as far as the entry knows it: the samples end with the x buffer (zeros beyond, which only a
            # ``last`` call may read)
            ref = self._shifted(xv, fv, f_first, k, n_ceps)
            out = [ref["log_env"], ref["ceps"]]
        else:
            out = [np.zeros((self.B, 0, nb)), np.zeros((self.B, 0, n_ceps))]
        out = [torch.tensor(np.ascontiguousarray(a)) for a in out]
        if full:
            return tuple(out)
        return out[0] if m.filter_order is None else out[1]

    def _shifted(self, xv, fv, f_first, k, n_ceps):
        """Frames f_first .. f_first + k - 1: the restatement takes frames from 0, so the frames before them get a harmless
        f0 and are cut away (a frame reads its own f0 only)."""
        m = self.module
        fv = fv.copy()
        fv[:, :f_first] = 0.0
        ref = env_ref.analyse(xv, fv[:, :f_first + k], m.sample_rate, self.hop, m.n_fft, n_ceps, m.f0_floor, m.f0_ceil,
                              m.unvoiced_f0, m.q1, m.eps, m.voiced_offset)
        return {key: ref[key][:, f_first:] for key in ("log_env", "ceps")}


# name -> (module arguments, T, F, f0 range): hop 1, hop 16 and a hop above the longest window
ENV_HOST_CASES = {
    "hop1": (dict(sample_rate=24000.0, hop_length=1, n_fft=64, f0_floor=3 * 24000 / 40.5, f0_ceil=6000.0, unvoiced_f0=3000.0),
             90, 41, (1500.0, 6500.0)),
    "hop16": (dict(sample_rate=24000.0, hop_length=16, n_fft=64, filter_order=9, f0_floor=3 * 24000 / 50.5, f0_ceil=6000.0,
                   unvoiced_f0=3000.0), 290, 20, (1200.0, 6500.0)),
    "hop80": (dict(sample_rate=24000.0, hop_length=80, n_fft=64, filter_order=4, f0_floor=3 * 24000 / 60.5, f0_ceil=6000.0,
                   unvoiced_f0=2000.0), 900, 11, (1000.0, 6500.0)),
}


def f0_track(B, F, lo, hi, rng):
    f0 = rng.uniform(lo, hi, (B, F)).astype(np.float32)
    f0[rng.uniform(size=(B, F)) < 0.3] = 0
    return f0


MODES = ["mixed", "controls first", "audio first"]


@pytest.mark.parametrize("name", list(ENV_HOST_CASES))
@pytest.mark.parametrize("mode", MODES)
def test_env_offset_indexing_against_the_float64_restatement(name, mode):
    kw, T, F, (lo, hi) = ENV_HOST_CASES[name]
    m = SpectralEnvelopeAnalysis(**kw)
    hop = kw["hop_length"]
    rng0 = np.random.default_rng(len(name))
    x, f0 = rng0.normal(0, 0.3, (2, T)).astype(np.float32), f0_track(2, F, lo, hi, rng0)
    n_ceps = 33 if m.filter_order is None else m.filter_order + 1
    ref = env_ref.analyse(x, f0, m.sample_rate, hop, 64, n_ceps, m.f0_floor, m.f0_ceil, m.unvoiced_f0)
    st = HostEnvStream(m, 2)
    assert st.hwmax == {"hop1": 20, "hop16": 25, "hop80": 30}[name] and ref["hw"].max() == st.hwmax

    def push(a, c):
        return [t.numpy() for t in st.push_all(x=None if a is None else torch.tensor(a),
                                               f0=None if c is None else AudioTensor(tensors(c)[0], hop))]

    for seed in (1, 2):   # the second utterance runs on the same stream, after finish()
        rng = np.random.default_rng(seed)
        got, counts = drive(push, lambda: [t.numpy() for t in st.finish_all()], x, [f0], rng,
                            [0, 1, 2, hop, st.span + 3, 2 * st.span + 1], [0, 1, 1, 2, 5], mode)
        assert sum(counts) == F
        assert np.array_equal(got[0], ref["log_env"]) and np.array_equal(got[1], ref["ceps"])
        assert (st.pushed, st.f0_received, st.framed) == (0, 0, 0)
    assert_exact_trimming(frame_calls(st.calls), lambda nxt, _: AS.env_keep_from(nxt, st.hwmax, hop))
    launches = [c for c in st.calls if c[5]]
    assert any(c[0] > 0 for c in launches) and any(c[3] > 0 for c in launches)   # a call above sample 0 and above frame 0
    if mode == "mixed" and name != "hop1":
        assert max(c[1] for c in st.calls) < T


class HostGlottalStream(_HostTake, AS.GlottalSourceStream):
    """``_frames`` is tests/hna_ref.py and tests/glottal_ref.py on the buffers laid out as golf_harmonic_analysis_stream_f32
    defines, the match on the f0 of exactly the frames asked for."""

    def __init__(self, module, batch_size):
        super().__init__(module, batch_size)
        self.calls = []
        self.plan = glottal_ref.plan(module.table.numpy(), module.num_harmonics)

    def _frames(self, e, f0, x_t0, f_first, f0_first, k, last, full):
        self.calls.append((x_t0, e.shape[1], f_first, f0_first, f0.shape[1], k, last))
        assert (x_t0 + e.shape[1], f0_first + f0.shape[1]) == (self.pushed, self.f0_received)
        if not k:
            return super()._frames(e, f0, x_t0, f_first, f0_first, k, last, full)   # launches nothing: no device is asked for
        with pytest.raises(GolfError, match="no CPU path"):
            super()._frames(e, f0, x_t0, f_first, f0_first, k, last, full)
        m = self.module
        ev, fv = laid_out(e, x_t0, np.nan), laid_out(f0, f0_first, 12345.0)
        with np.errstate(all="ignore"):
            h = hna_ref.analyse(ev, fv, m.sample_rate, self.hop, m.num_harmonics, 0, m.periods, m.min_window, m.max_window,
                                self.unvoiced_window)
        sl = slice(f_first, f_first + k)
        r = glottal_ref.match(h["amp"][:, sl].astype(np.float32), h["phase"][:, sl].astype(np.float32), fv[:, sl], *self.plan,
                              m.sample_rate, m.n_phi)
        w = np.where(np.isnan(r["w"]), m.unvoiced_weight, r["w"])
        return tuple(torch.tensor(np.ascontiguousarray(a)) for a in (w, r["theta"], r["rho"]))


GLOTTAL_HOST_CASES = {
    "hop1": (dict(sample_rate=24000.0, hop_length=1, num_harmonics=3, n_phi=16, min_window=2, max_window=17), 37, 41,
             (6000.0, 11000.0)),
    "hop16": (dict(sample_rate=24000.0, hop_length=16, num_harmonics=3, n_phi=16, min_window=32, max_window=48), 290, 20,
              (1500.0, 3000.0)),
    "hop80": (dict(sample_rate=24000.0, hop_length=80, num_harmonics=2, n_phi=8, min_window=8, max_window=33), 2400, 31,
              (3000.0, 6000.0)),
}


@pytest.mark.parametrize("name", list(GLOTTAL_HOST_CASES))
@pytest.mark.parametrize("mode", MODES)
def test_glottal_offset_indexing_against_the_float64_restatement(name, mode):
    kw, T, F, (lo, hi) = GLOTTAL_HOST_CASES[name]
    table = torch.tensor(np.random.default_rng(3).normal(0, 1, (5, 32)).astype(np.float32))
    m = GlottalSourceAnalysis(table, unvoiced_weight=0.25, **kw)
    hop = kw["hop_length"]
    rng0 = np.random.default_rng(len(name) + 7)
    e, f0 = rng0.normal(0, 0.3, (2, T)).astype(np.float32), f0_track(2, F, lo, hi, rng0)
    st = HostGlottalStream(m, 2)
    assert st.span == max(kw["max_window"], 4 * hop)
    with np.errstate(all="ignore"):
        h = hna_ref.analyse(e, f0, m.sample_rate, hop, m.num_harmonics, 0, m.periods, m.min_window, m.max_window, 4 * hop)
    r = glottal_ref.match(h["amp"].astype(np.float32), h["phase"].astype(np.float32), f0, *st.plan, m.sample_rate, m.n_phi)
    assert np.isnan(r["w"]).any() and not np.isnan(r["w"]).all()
    want = [np.where(np.isnan(r["w"]), 0.25, r["w"]), r["theta"], r["rho"]]

    def push(a, c):
        return [t.numpy() for t in st.push_all(e=None if a is None else AudioTensor(torch.tensor(a)),
                                               f0=None if c is None else tensors(c)[0])]

    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        got, counts = drive(push, lambda: [t.numpy() for t in st.finish_all()], e, [f0], rng,
                            [0, 1, 2, hop, st.span + 3, 2 * st.span + 1], [0, 1, 1, 2, 5], mode)
        assert sum(counts) == F and len(got) == 3
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w)
        assert (st.pushed, st.f0_received, st.framed) == (0, 0, 0)
    assert_exact_trimming(frame_calls(st.calls), lambda nxt, _: AS.hna_keep_from(nxt, st.span, hop))
    launches = [c for c in st.calls if c[5]]
    assert any(c[0] > 0 for c in launches) and any(c[3] > 0 for c in launches)
    assert any(c[5] == 0 for c in st.calls)   # and a push that completed no frame asked for no device
    if mode == "mixed" and name != "hop1":
        assert max(c[1] for c in st.calls) < T


class HostResidualStream(AS.ResidualStream):
    """The stream with the device left out: every check of a push is made and then the CPU tensors are accepted, and
    ``_samples`` is tests/residual_ref.py on the buffers laid out as golf_ltv_residual_stream_f32 defines."""

    def __init__(self, hop, order, batch_size):
        super().__init__(hop, order, batch_size)
        self.calls = []

    def _device(self):
        return torch.device("cpu")

    def _require_device(self, *tensors):
        if any(t is not None for t in tensors):   # finish() brings none
            with pytest.raises(GolfError, match="no CPU path"):
                super()._require_device(*tensors)

    def _samples(self, x, gain, a, x_t0, fr_first, t_first, n, last):
        self.calls.append((x_t0, 0 if x is None else x.shape[1], fr_first, 0 if gain is None else gain.shape[1], t_first, n,
                           last))
        assert (x_t0 + self.calls[-1][1], fr_first + self.calls[-1][3]) == (self.pushed, self.frames_received)
        if not n:
            return super()._samples(x, gain, a, x_t0, fr_first, t_first, n, last).double()
        with pytest.raises(GolfError, match="no CPU path"):
            super()._samples(x, gain, a, x_t0, fr_first, t_first, n, last)
        out = residual_ref.residual(laid_out(x, x_t0, np.nan), laid_out(gain, fr_first, np.nan), laid_out(a, fr_first, np.nan),
                                    self.hop, t_first, n, last)
        return torch.tensor(out)


# (hop, M, F, T): T below, at and above (F - 1) hop + 1
RES_HOST_CASES = {"hop1": (1, 64, 130, 120), "hop3": (3, 33, 30, 88), "hop16": (16, 22, 20, 330), "hop80": (80, 7, 11, 801)}


@pytest.mark.parametrize("name", list(RES_HOST_CASES))
@pytest.mark.parametrize("mode", MODES)
def test_residual_offset_indexing_against_the_float64_restatement(name, mode):
    hop, M, F, T = RES_HOST_CASES[name]
    x, gain, a = residual_ref.inputs(2, F, M, T, seed=hop)
    want = residual_ref.residual(x, gain, a, hop)
    assert want.shape == (2, residual_ref.length(T, F, hop)) and np.isfinite(want).all()
    st = HostResidualStream(hop, M, 2)

    def push(blk, c):
        c = tensors(c)
        return [st.push(x=None if blk is None else torch.tensor(blk), gain=None if c is None else AudioTensor(c[0], hop),
                        a=None if c is None else c[1]).numpy()]

    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        got, counts = drive(push, lambda: [st.finish().numpy()], x, [gain, a], rng, [0, 1, 2, hop, M + 3, 5 * hop + 1],
                            [0, 1, 1, 2, 5], mode)
        assert sum(counts) == want.shape[1]
        assert np.array_equal(got[0], want)
        assert (st.pushed, st.frames_received, st.emitted) == (0, 0, 0)
    assert_exact_trimming([(x_t0, n_x, t_first, fr_first, n_fr, last) for x_t0, n_x, fr_first, n_fr, t_first, n, last in st.calls],
                          lambda emitted, frames: AS.res_keep_from(emitted, frames, M, hop))
    launches = [c for c in st.calls if c[5]]
    assert len(launches) >= 3 or mode != "mixed"
    assert any(c[0] > 0 for c in launches) and any(c[2] > 0 for c in launches)   # above sample 0 and above frame 0
    if mode == "mixed" and name != "hop1":
        assert max(c[1] for c in st.calls) < T and max(c[3] for c in st.calls) < F


def test_residual_counts_at_finish():
    """finish() emits min(T, (F - 1) hop + 1) samples in all for T far below, equal to and far above (F - 1) hop; none when
    F = 0; one, x[0] / gain[0], when F = 1."""
    hop, M, F = 16, 5, 6
    for T in (0, 3, (F - 1) * hop, (F - 1) * hop + 1, (F - 1) * hop + 500):
        x, gain, a = residual_ref.inputs(2, F, M, T, seed=T)
        st = HostResidualStream(hop, M, 2)
        first = st.push(torch.tensor(x), torch.tensor(gain), torch.tensor(a))
        rest = st.finish()
        assert first.shape == (2, AS.res_samples_final(T, F, hop)) == (2, min(T, (F - 1) * hop))
        assert rest.shape == (2, residual_ref.length(T, F, hop) - first.shape[1])
        assert np.array_equal(torch.cat([first, rest], 1).numpy(), residual_ref.residual(x, gain, a, hop))
        assert rest.shape[1] == (1 if T > (F - 1) * hop else 0)   # the clamped last sample comes out at finish() only
    st = HostResidualStream(hop, M, 2)
    assert st.push(x=torch.zeros(2, 500)).shape == (2, 0) and st.finish().shape == (2, 0)   # F = 0
    x, gain, a = residual_ref.inputs(2, 1, M, 40, seed=1)
    assert st.push(torch.tensor(x), torch.tensor(gain), torch.tensor(a)).shape == (2, 0)
    one = st.finish()
    assert one.shape == (2, 1) and np.array_equal(one.numpy()[:, 0], x[:, 0].astype(np.float64) / gain[:, 0])


def test_env_and_glottal_counts_at_finish():
    """push / finish return what forward returns; finish() emits one frame per f0 frame whatever T."""
    kw, _, F, (lo, hi) = ENV_HOST_CASES["hop16"]
    m = SpectralEnvelopeAnalysis(**kw)
    gkw = GLOTTAL_HOST_CASES["hop16"][0]
    table = torch.tensor(np.random.default_rng(3).normal(0, 1, (5, 32)).astype(np.float32))
    gm = GlottalSourceAnalysis(table, **gkw)
    for T in (0, 5, (F - 1) * 16, (F - 1) * 16 + 1, (F - 1) * 16 + 1000):
        rng = np.random.default_rng(T)
        x, f0 = rng.normal(0, 0.3, (2, T)).astype(np.float32), f0_track(2, F, lo, hi, rng)
        ref = env_ref.analyse(x, f0, m.sample_rate, 16, 64, 10, m.f0_floor, m.f0_ceil, m.unvoiced_f0)
        st = HostEnvStream(m, 2)
        first, rest = st.push(torch.tensor(x), torch.tensor(f0)), st.finish()
        assert all(isinstance(t, AudioTensor) and t.hop_length == 16 for t in (first, rest))
        n_first = AS.env_frames_final(T, F, st.hwmax, 16)
        assert first.shape == (2, n_first, 10) and rest.shape == (2, F - n_first, 10)
        assert np.array_equal(torch.cat([first.as_tensor(), rest.as_tensor()], 1).numpy(), ref["ceps"])
        gs = HostGlottalStream(gm, 2)
        first, rest = gs.push(torch.tensor(x), torch.tensor(f0 * 1.5)), gs.finish()
        assert all(isinstance(t, AudioTensor) and t.hop_length == 16 for t in (first, rest))
        n_first = AS.hna_frames_final(T, F, 64, 16)
        assert first.shape == (2, n_first) and rest.shape == (2, F - n_first)
    for st, shapes in ((HostEnvStream(m, 2), [(2, 0, 33), (2, 0, 10)]), (HostGlottalStream(gm, 2), [(2, 0)] * 3)):
        st.push(torch.zeros(2, 500))   # no f0 frame at all: empty results, whatever audio came
        assert [tuple(t.shape) for t in st.finish_all()] == shapes
    only = HostEnvStream(SpectralEnvelopeAnalysis(**ENV_HOST_CASES["hop1"][0]), 1)   # log_env when filter_order is None
    out = only.push(torch.zeros(1, 200), torch.full((1, 3), 3000.0))
    assert isinstance(out, AudioTensor) and out.shape == (1, 3, 33) and only.finish().shape == (1, 0, 33)


# ---- refusals without a device -----------------------------------------------------------------------------------------------
def test_env_functional_refuses_before_a_launch():
    assert {"spectral_envelope_stream", "ltv_residual", "ltv_residual_stream"} <= set(GF.__all__)
    x, f0 = torch.zeros(2, 3000), torch.full((2, 12), 100.0)
    base = dict(x_t0=0, f_first=0, f0_first=0, n_frames=8, last=False, sample_rate=24000, hop=240, n_ceps=40)

    def call(x=x, f0=f0, **kw):
        return GF.spectral_envelope_stream(x, f0, **dict(base, **kw))

    for kw in (dict(), dict(n_frames=0), dict(x=x[:0], f0=f0[:0])):   # everything holds: only the device is missing
        with pytest.raises(GolfError, match="no CPU path"):
            call(**kw)
    with pytest.raises(GolfError, match="must be \\(B, T\\)"):
        call(x=torch.zeros(3000))
    with pytest.raises(GolfError, match="f0 must be \\(B, F\\)"):
        call(f0=f0[:1])
    # hwmax = 511: frame 5 may start at sample 689 and frame 8 may end at sample 2431 (2432 samples)
    for kw, what in ((dict(hop=0), "hop"), (dict(n_fft=1000), "n_fft"), (dict(n_ceps=514), "n_ceps"), (dict(sample_rate=0), "sample_rate"),
                     (dict(eps=0), "eps"), (dict(f0_floor=10.0), "f0_floor"), (dict(f0_ceil=7000.0), "f0_ceil"),
                     (dict(unvoiced_f0=10.0), "unvoiced_f0"), (dict(q1=float("nan")), "q1"),
                     (dict(n_ceps=None, return_log_env=False), "nothing to return"),
                     (dict(n_frames=-1), "n_frames"), (dict(x_t0=-1), "x_t0"), (dict(f0_first=-1), "f0_first"),
                     (dict(f_first=-1), "f_first"), (dict(f_first=2 ** 61), "f_first"),
                     (dict(f_first=5, n_frames=4, x_t0=690), "x_t0"), (dict(f_first=5, n_frames=4, f0_first=6), "f0_first"),
                     (dict(f_first=0, f0_first=1), "f0_first"), (dict(n_frames=13, last=True), "n_f0"),
                     (dict(n_frames=12), "n_x"), (dict(f_first=5, n_frames=4, x_t0=689, x=x[:, :1742]), "n_x")):
        with pytest.raises(GolfError, match=what):
            call(**kw)
    # the same windows are accepted at their limits
    for kw in (dict(f_first=5, n_frames=4, x_t0=689, f0_first=5, x=x[:, :1743], f0=f0[:, :4]),
               dict(f_first=5, n_frames=7, x_t0=689, f0_first=5, x=x[:, :1], f0=f0[:, :7], last=True),
               dict(n_frames=11), dict(n_frames=12, last=True, x=x[:, :0])):
        with pytest.raises(GolfError, match="no CPU path"):
            call(**kw)


def test_env_c_entry_refuses_before_a_launch():
    from golf_amd import _lib

    lib = _lib.load()
    assert "golf_spectral_envelope_stream_f32" in _lib.SIGNATURES and lib.golf_abi_version() == 6
    EINVAL, EUNSUPPORTED, fake = -1, -3, 256   # the pointers are never dereferenced
    lo, hi = GF.spectral_envelope_defaults(24000.0, 1024)

    def call(x=fake, xs=None, x_t0=689, n_x=1743, f0=fake, fs=None, f0_first=5, n_f0=4, env=fake, ceps=fake, B=2, f_first=5,
             n_frames=4, last=0, n_fft=1024, n_ceps=40, hop=240, sr=24000.0, lo=lo, hi=hi, uv=500.0, q1=-0.15, eps=1e-12,
             off=0.3):
        rc = lib.golf_spectral_envelope_stream_f32(x, n_x if xs is None else xs, x_t0, n_x, f0, n_f0 if fs is None else fs,
                                                   f0_first, n_f0, env, ceps, B, f_first, n_frames, last, n_fft, n_ceps, hop,
                                                   sr, lo, hi, uv, q1, eps, off, None)
        if rc:
            assert b"spectral_envelope_stream" in lib.golf_last_error()
        return rc

    assert call(n_fft=1000) == EUNSUPPORTED and b"n_fft" in lib.golf_last_error()
    for kw, word in ((dict(x=None), b"null"), (dict(f0=None), b"null"), (dict(env=None, ceps=None), b"null"),
                     (dict(n_ceps=0), b"n_ceps"), (dict(B=0), b"size"), (dict(n_x=-1), b"size"), (dict(n_f0=0), b"size"),
                     (dict(n_frames=0), b"size"), (dict(xs=1742), b"stride"), (dict(fs=3), b"stride"), (dict(hop=0), b"hop"),
                     (dict(sr=0.0), b"sample_rate"), (dict(eps=0.0), b"eps"), (dict(n_ceps=514), b"n_ceps"),
                     (dict(lo=0.0), b"f0_floor"), (dict(lo=3000.0), b"f0_floor"), (dict(hi=7000.0), b"f0_ceil"),
                     (dict(uv=10.0), b"unvoiced_f0"), (dict(q1=float("nan")), b"q1"), (dict(lo=10.0, uv=500.0), b"f0_floor"),
                     (dict(B=1 << 20, n_frames=1 << 11), b"2^31"), (dict(x_t0=-1), b"x_t0"), (dict(f0_first=-1), b"f0_first"),
                     (dict(f_first=-1), b"f_first"), (dict(f_first=1 << 61), b"f_first"),
                     # the preconditions of the position: each one step beyond its limit
                     (dict(x_t0=690, n_x=1742), b"x_t0"), (dict(f0_first=6, n_f0=3), b"f0_first"),
                     (dict(f_first=0, x_t0=0, f0_first=1), b"f0_first"), (dict(n_f0=3), b"n_f0"), (dict(n_f0=3, last=1), b"n_f0"),
                     (dict(n_x=1742), b"n_x")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())
    call(n_x=1742)
    assert b"last is not set" in lib.golf_last_error()


def test_residual_functional_refuses_before_a_launch():
    x, gain, a = torch.zeros(2, 3000), torch.ones(2, 12), torch.zeros(2, 12, 22)
    base = dict(x_t0=0, fr_first=0, t_first=0, n_out=2000, last=False, hop=240)

    def call(x=x, gain=gain, a=a, **kw):
        return GF.ltv_residual_stream(x, gain, a, **dict(base, **kw))

    for kw in (dict(), dict(n_out=0), dict(x=x[:0], gain=gain[:0], a=a[:0])):
        with pytest.raises(GolfError, match="no CPU path"):
            call(**kw)
    for args in ((x, gain, a), (x[:0], gain[:0], a[:0]), (x[:, :0], gain, a)):
        with pytest.raises(GolfError, match="no CPU path"):
            GF.ltv_residual(*args, 240)
    for args, what in (((x[0], gain, a), "must be \\(B, T\\)"), ((x, gain[:1], a), "gain must be"), ((x, gain, a[:, :5]), "a must be"),
                       ((x, gain, torch.zeros(2, 12, 65)), "M=65"), ((x, gain, torch.zeros(2, 12, 0)), "M=0"),
                       ((x, gain[:, :0], a[:, :0]), "frames")):
        with pytest.raises(GolfError, match=what):
            GF.ltv_residual(*args, 240)
    with pytest.raises(GolfError, match="hop"):
        GF.ltv_residual(x, gain, a, 0)
    # M = 22: sample 1000 reads from sample 978 and frames 4 and 5; samples 1000..1999 need frame 9
    for kw, what in ((dict(hop=0), "hop"), (dict(a=torch.zeros(2, 12, 65)), "M=65"), (dict(n_out=-1), "n_out"),
                     (dict(x_t0=-1), "x_t0"), (dict(t_first=-1), "t_first"), (dict(fr_first=-1), "fr_first"),
                     (dict(fr_first=2 ** 61), "fr_first"), (dict(t_first=2 ** 63), "t_first"),
                     (dict(t_first=1000, n_out=1000, x_t0=979), "x_t0"), (dict(t_first=5, n_out=10, x_t0=1), "x_t0"),
                     (dict(n_out=3001), "n_x"), (dict(t_first=1000, n_out=1000, x_t0=978, x=x[:, :1021]), "n_x"),
                     (dict(t_first=1000, n_out=1000, fr_first=5), "fr_first"),
                     (dict(t_first=1000, n_out=1000, fr_first=4, gain=gain[:, :5], a=a[:, :5]), "n_fr"),
                     (dict(n_out=2641), "n_fr"),                                  # sample 2640 needs frame 12
                     (dict(n_out=2642, last=True), "n_out"),                      # (F - 1) hop + 1 = 2641
                     (dict(t_first=2640, n_out=1, fr_first=11, last=True, gain=gain[:, :1], a=a[:, :1]), "fr_first"),   # the clamp: frame 10 is read
                     (dict(t_first=0, n_out=1, fr_first=1, last=True, gain=gain[:, :1], a=a[:, :1]), "fr_first")):   # F = 2 here: frame 0
        with pytest.raises(GolfError, match=what):
            call(**kw)
    for kw in (dict(t_first=1000, n_out=1000, x_t0=978, fr_first=4, x=x[:, :1022], gain=gain[:, :6], a=a[:, :6]),
               dict(n_out=2640), dict(n_out=2641, last=True), dict(t_first=2640, n_out=1, fr_first=10, x_t0=2618, last=True,
                                                                 x=x[:, :23], gain=gain[:, :2], a=a[:, :2]),
               dict(n_out=1, last=True, gain=gain[:, :1], a=a[:, :1])):           # F = 1: one sample
        with pytest.raises(GolfError, match="no CPU path"):
            call(**kw)


def test_residual_c_entries_refuse_before_a_launch():
    from golf_amd import _lib

    lib = _lib.load()
    assert {"golf_ltv_residual_f32", "golf_ltv_residual_stream_f32"} <= set(_lib.SIGNATURES)
    EINVAL, fake = -1, 256

    def one(x=fake, xs=3000, gain=fake, a=fake, e=fake, es=2641, B=2, T=3000, F=12, M=22, hop=240):
        rc = lib.golf_ltv_residual_f32(x, xs, gain, a, e, es, B, T, F, M, hop, None)
        if rc:
            assert b"ltv_residual:" in lib.golf_last_error()
        return rc

    for kw, word in ((dict(x=None), b"null"), (dict(gain=None), b"null"), (dict(a=None), b"null"), (dict(e=None), b"null"),
                     (dict(B=0), b"size"), (dict(T=0), b"size"), (dict(F=0), b"size"), (dict(M=0), b"M=0"), (dict(M=65), b"M=65"),
                     (dict(hop=0), b"hop"), (dict(xs=2999), b"stride"), (dict(es=2640), b"stride"),
                     (dict(T=100, es=99), b"stride"), (dict(B=1 << 24, T=1 << 20, F=1 << 20, xs=1 << 20, es=1 << 20), b"2^31")):
        assert one(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())

    def call(x=fake, xs=None, x_t0=978, n_x=1022, gain=fake, a=fake, fr_first=4, n_fr=6, e=fake, es=None, B=2, t_first=1000,
             n_out=1000, last=0, M=22, hop=240):
        rc = lib.golf_ltv_residual_stream_f32(x, n_x if xs is None else xs, x_t0, n_x, gain, a, fr_first, n_fr, e,
                                              n_out if es is None else es, B, t_first, n_out, last, M, hop, None)
        if rc:
            assert b"ltv_residual_stream" in lib.golf_last_error()
        return rc

    for kw, word in ((dict(x=None), b"null"), (dict(gain=None), b"null"), (dict(a=None), b"null"), (dict(e=None), b"null"),
                     (dict(B=0), b"size"), (dict(n_x=0), b"size"), (dict(n_fr=0), b"size"), (dict(n_out=0), b"size"),
                     (dict(M=0), b"M=0"), (dict(M=65), b"M=65"), (dict(hop=0), b"hop"), (dict(xs=1021), b"stride"),
                     (dict(es=999), b"stride"), (dict(x_t0=-1), b"x_t0"), (dict(x_t0=(1 << 62) + 1), b"x_t0"),
                     (dict(t_first=-1), b"t_first"), (dict(t_first=(1 << 62) + 1), b"t_first"), (dict(fr_first=-1), b"fr_first"),
                     (dict(fr_first=1 << 61), b"fr_first"),
                     # the preconditions of the position: each one step beyond its limit
                     (dict(x_t0=979, n_x=1021), b"x_t0"), (dict(t_first=5, n_out=10, x_t0=1, n_x=14, fr_first=0), b"x_t0"),
                     (dict(n_x=1021), b"n_x"), (dict(fr_first=5, n_fr=5), b"fr_first"), (dict(n_fr=5), b"n_fr"),
                     (dict(n_fr=5, last=1), b"n_out"),                  # F = 9: the samples would end beyond 8 hop + 1 = 1921
                     (dict(t_first=2640, n_out=1, x_t0=2618, n_x=23, fr_first=11, n_fr=1, last=1), b"fr_first")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())
    call(n_fr=5)
    assert b"last is not set" in lib.golf_last_error()


def test_stream_surface_without_a_device():
    from golf_amd.f0 import F0Analysis

    assert {"SpectralEnvelopeStream", "GlottalSourceStream", "ResidualStream", "env_frames_final", "env_keep_from",
            "res_samples_final", "res_keep_from"} <= set(AS.__all__)
    em = SpectralEnvelopeAnalysis(24000, 240, filter_order=80)
    gm = GlottalSourceAnalysis(torch.randn(4, 64), 24000, 240)
    with pytest.raises(TypeError, match="SpectralEnvelopeAnalysis is needed"):
        AS.SpectralEnvelopeStream(gm, 3)
    with pytest.raises(TypeError, match="GlottalSourceAnalysis is needed"):
        AS.GlottalSourceStream(F0Analysis(24000, 240), 3)
    for make in (lambda B: AS.SpectralEnvelopeStream(em, B), lambda B: AS.GlottalSourceStream(gm, B),
                 lambda B: AS.ResidualStream(240, 22, B)):
        with pytest.raises(ValueError, match="batch_size"):
            make(0)
    with pytest.raises(GolfError, match="lpc_order"):
        AS.ResidualStream(240, 65, 3)
    with pytest.raises(GolfError, match="hop"):
        AS.ResidualStream(0, 22, 3)
    x, f0 = torch.zeros(3, 100), torch.zeros(3, 2)
    for st, audio in ((AS.SpectralEnvelopeStream(em, 3), "x"), (AS.GlottalSourceStream(gm, 3), "e")):
        with pytest.raises(NotImplementedError, match="requires grad"):
            st.push(**{audio: x.clone().requires_grad_(True)})
        with pytest.raises(NotImplementedError, match="requires grad"):
            st.push(f0=f0.clone().requires_grad_(True))
        with pytest.raises(ValueError, match="B=3"):
            st.push(**{audio: x[:2]})
        with pytest.raises(ValueError, match="B=3"):
            st.push(f0=f0[:2])
        with pytest.raises(AssertionError, match="hop 1"):
            st.push(**{audio: AudioTensor(x, 2)})
        with pytest.raises(AssertionError, match="hop 240"):
            st.push(f0=AudioTensor(f0, 120))
        for kw in ({audio: x}, dict(f0=f0), {audio: x, "f0": f0}, {audio: x.double()}):
            with pytest.raises(GolfError, match="no CPU path"):
                st.push(**kw)
        assert (st.pushed, st.f0_received, st.framed) == (0, 0, 0)   # a refused push leaves the stream as it was
    st = AS.ResidualStream(240, 22, 3)
    gain, a = torch.ones(3, 2), torch.zeros(3, 2, 22)
    with pytest.raises(ValueError, match="come together"):
        st.push(gain=gain)
    with pytest.raises(ValueError, match="lpc_order=22"):
        st.push(gain=gain, a=a[:, :, :5])
    with pytest.raises(ValueError, match="beside gain"):
        st.push(gain=gain, a=a[:, :1])
    with pytest.raises(ValueError, match="B=3"):
        st.push(x=x[:2])
    with pytest.raises(ValueError, match="B=3"):
        st.push(gain=gain, a=a[0])
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(gain=gain, a=a.clone().requires_grad_(True))
    with pytest.raises(AssertionError, match="hop 240"):
        st.push(gain=AudioTensor(gain, 120), a=a)
    for kw in (dict(x=x), dict(gain=gain, a=a), dict(x=x, gain=gain, a=a)):
        with pytest.raises(GolfError, match="no CPU path"):
            st.push(**kw)
    assert (st.pushed, st.frames_received, st.emitted) == (0, 0, 0)
