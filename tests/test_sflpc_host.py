"""CPU: the host side of the source-compensated LPC analysis -- the float64 restatement (tests/sflpc_ref.py) against what it
restates (lags of a filtered frame against the autocorrelation of the convolution; ``preemphasis=0, iterations=0`` against
tests/lpc_analysis_ref.py), its stability, what it is worth to the glottal-source analysis on the planted construction of
tools/glottal_preemphasis.py, and the module, the stream and the C entry's argument checks without a GPU."""
import numpy as np
import pytest
import torch

import lpc_analysis_ref as L
import sflpc_ref as S


@pytest.mark.parametrize("P", (1, 4, 22))
def test_lags_of_a_filtered_frame(P):
    """With eps = 0, (r o c)[j] is the autocorrelation of the full convolution s * c: 1e-12 of the largest lag."""
    W, n = 50, 22
    rng = np.random.default_rng(P)
    s = rng.normal(0, 1, W)
    c = np.concatenate([[1.0], rng.normal(0, 0.5, P)])
    r = torch.tensor([s[: W - j] @ s[j:] for j in range(n + P + 1)])
    got = S.filtered_lags(r, torch.tensor(c), n).numpy()
    y = np.convolve(s, c)
    want = np.array([y[: len(y) - j] @ y[j:] for j in range(n + 1)])
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"P={P}: {err:.2e}")
    assert err <= 1e-12


def test_without_a_source_model_it_is_the_plain_analysis(golden):
    """preemphasis=0, iterations=0: a and rc are exactly lpc_analysis_ref.analysis's, the gain -- (r o a)[0] against E_M, two
    float64 expressions of the same number -- agrees to 1e-12."""
    x = np.concatenate([L.speech_like(golden, (0, 9), 2400), np.random.default_rng(2).normal(0, 1, (1, 2400))])
    x[1, 400:2100] = 0.0
    w = torch.hann_window(960, dtype=torch.float64)
    gain0, a0, rc0 = L.analysis(x, w, 240, 22)
    gain, a, rc, source = S.analysis(x, w, 240, 22, 4, 0, 0.0)
    assert torch.equal(a, a0) and torch.equal(rc, rc0) and torch.all(source == 0) and source.shape == (3, 11, 4)
    err = ((gain - gain0).abs() / gain0).max()
    print(f"gain {err:.2e}  max |rc| {rc.abs().max():.4f}")
    assert err <= 1e-12
    assert (a[1].abs().amax(-1) == 0).sum() >= 2   # silent frames: a = 0, as today


@pytest.mark.parametrize("kw", (dict(), dict(preemphasis=0.97), dict(Q=8, iterations=3), dict(Q=1, iterations=0)))
def test_stability(golden, kw):
    """|rc| < 1 and rc2lpc(rc) == a on audio with the conditioning of speech, whatever the stages before the last."""
    from oracle import golf_oracle as O

    x = L.speech_like(golden, (0, 9, 4), 2400)
    gain, a, rc, source = S.analysis(x, torch.hann_window(960, dtype=torch.float64), 240, 22, **kw)
    assert all(torch.isfinite(t).all() for t in (gain, a, rc, source)) and (gain > 0).all()
    err = np.abs(O.rc2lpc(rc.numpy()) - a.numpy()).max()
    print(f"{kw}: max |rc| {rc.abs().max():.5f}  rc2lpc {err:.2e}")
    assert rc.abs().max() < 1.0 and err <= 1e-12


def test_worth_on_the_planted_case():
    """Pulses of the package's table at a constant table position w through the fixed 5-formant filter, 40 frames of one row:
    the analysis of the audio -> residual -> harmonics -> match, error of w in table steps on interior frames (max / rms) and
    the rms of the residual (the planted excitation's is 0.996 / 0.998).  Measured when this was written:

        analysis of the audio                          w = 0.3       w = 0.7      rms(e)
        plain (lpc_analysis_ref)                       6.67 / 4.15   3.03 / 1.37  0.652 / 0.648
        plain, of 0.97-pre-emphasised audio            2.46 / 1.58   1.50 / 0.94  3.100 / 3.737
        preemphasis=0.97, iterations=0                 1.76 / 0.85   1.72 / 0.99  0.993 / 1.003
        adaptive first stage, iterations=0             1.40 / 0.71   1.92 / 0.99  0.993 / 1.005
        source_order=4, iterations=2 (the default)     1.56 / 0.93   1.98 / 0.79  0.991 / 1.003
        source_order=4, iterations=3                   1.95 / 0.95   2.05 / 0.67  0.990 / 1.003
        preemphasis=0, iterations=0                    = plain       = plain      0.652 / 0.648
        the true inverse filter                        0.70 / 0.44   0.58 / 0.30

    The default must beat the plain analysis strictly and be no worse than the plain analysis of pre-emphasised audio, in the
    rms error of w at both positions; both baselines come from lpc_analysis_ref.  Its residual has the planted excitation's
    rms within 2 %."""
    win = torch.hann_window(S.WINDOW, dtype=torch.float64)   # periodic
    rows = (("preemphasis=0.97, iterations=0", dict(preemphasis=0.97, iterations=0)),
            ("adaptive first stage, iterations=0", dict(iterations=0)),
            ("source_order=4, iterations=2", dict()),
            ("source_order=4, iterations=3", dict(iterations=3)),
            ("preemphasis=0, iterations=0", dict(preemphasis=0.0, iterations=0)))
    for w0 in (0.3, 0.7):
        pl = S.planted(w0)
        y = torch.tensor(pl["y"])[None]
        assert y.shape == (1, 39 * S.HOP + 1)
        gain, a, _ = L.analysis(y, win, S.HOP, S.ORDER)
        plain = S.planted_score(pl, gain, a)
        gain, a, _ = L.analysis(torch.tensor(S.preemphasised(pl["y"]))[None], win, S.HOP, S.ORDER)
        pre = S.planted_score(pl, gain, a)
        true = S.worth(pl, np.convolve(pl["y"], S.allpole())[None, :len(pl["y"])])
        e_rms = S.rms(pl["e"])
        print(f"w = {w0}: planted excitation rms {e_rms:.3f}; the true inverse filter {true[0]:.2f} / {true[1]:.2f}")
        print(f"  {'plain':42s} {plain[0]:.2f} / {plain[1]:.2f}  rms(e) {plain[2]:.3f}")
        print(f"  {'plain, of 0.97-pre-emphasised audio':42s} {pre[0]:.2f} / {pre[1]:.2f}  rms(e) {pre[2]:.3f}")
        got = {}
        for label, kw in rows:
            gain, a, _, _ = S.analysis(y, win, S.HOP, S.ORDER, **kw)
            got[label] = S.planted_score(pl, gain, a)
            print(f"  {label:42s} {got[label][0]:.2f} / {got[label][1]:.2f}  rms(e) {got[label][2]:.3f}")
        default = got["source_order=4, iterations=2"]
        assert default[1] < plain[1] and default[1] <= pre[1]
        assert abs(default[2] - e_rms) <= 0.02 * e_rms
        assert true[1] < default[1]   # the case is what it claims to be: there is room below


def test_module_and_stream_surface():
    from golf_amd import analysis_stream as AS
    from golf_amd import functional as GF
    from golf_amd import lpc
    from golf_amd._lib import GolfError
    from golf_amd.lpc import LPCAnalysis, SourceFilterLPCAnalysis

    assert "SourceFilterLPCAnalysis" in lpc.__all__ and "source_filter_lpc" in GF.__all__
    assert "SourceFilterLPCStream" in AS.__all__
    m = SourceFilterLPCAnalysis(22, 240)
    assert not isinstance(m, LPCAnalysis)   # a sibling: LPCAnalysisStream dispatches on the type
    assert (m.window_length, m.source_order, m.iterations, m.preemphasis, m.centred) == (960, 4, 2, None, True)
    assert m._window.shape == (960,) and m._window.dtype == torch.float32 and not m.state_dict()
    with pytest.raises(GolfError, match="no CPU path"):
        m(torch.zeros(1, 1000))
    with pytest.raises(GolfError, match="no CPU path"):
        m.logits(torch.zeros(1, 1000))
    st = AS.open_analysis_stream(m, 2, return_rc=True, return_source=True)
    assert type(st) is AS.SourceFilterLPCStream and st.return_rc and st.return_source and st.latency == 480
    assert type(AS.open_analysis_stream(LPCAnalysis(22, 240), 2)) is AS.LPCAnalysisStream
    with pytest.raises(TypeError, match="an LPCAnalysis is needed"):
        AS.LPCAnalysisStream(m, 2)
    with pytest.raises(TypeError, match="SourceFilterLPCAnalysis is needed"):
        AS.SourceFilterLPCStream(LPCAnalysis(22, 240), 2)
    with pytest.raises(ValueError, match="batch_size"):
        AS.SourceFilterLPCStream(m, 0)
    with pytest.raises(GolfError, match="no CPU path"):
        st.push(torch.zeros(2, 100))


@pytest.mark.parametrize("centred", (True, False))
@pytest.mark.parametrize("span,hop", [(8, 3), (4, 9)])   # hop below and above the span
def test_stream_bookkeeping_on_the_host(span, hop, centred):
    """SourceFilterLPCStream over the frame-local stand-in of tests/test_f0_stream_host.py: random cuts of two utterances
    give what the stand-in gives on the whole zero-padded utterance, four results wide."""
    from golf_amd import analysis_stream as AS
    from golf_amd.lpc import SourceFilterLPCAnalysis
    from test_f0_stream_host import _host_frames, local_frames

    class Host(_host_frames(AS.SourceFilterLPCStream)):
        def _shape(self, out):
            return out, torch.stack([out + 1, out + 2], -1), torch.stack([out + 3, out + 4], -1), \
                torch.stack([out + 5, out + 6, out + 7], -1)

    B = 2
    st = Host(SourceFilterLPCAnalysis(2, hop, window_length=span, centred=centred, source_order=3), B, return_rc=True,
              return_source=True)
    for i, T in enumerate((0, span - 1, 5 * hop + span + 1)):
        rng = np.random.default_rng(100 * span + i)
        x = torch.tensor(rng.integers(-8, 9, (B, T)).astype(np.float32))
        F = AS.frames_final(T, span, hop, centred)
        want = st._shape(local_frames(torch.nn.functional.pad(x, (span // 2 if centred else 0, 0)), F, span, hop))
        parts, t = [], 0
        while t < T:
            n = int(rng.integers(0, 2 * hop + 2))
            st.block = min(n, T - t)
            parts.append(st.push_all(x[:, t:t + n]))
            t += n
        st.block = 0
        parts.append(st.finish_all())
        assert [p.shape[-1] for p in parts[0][1:]] == [2, 2, 3]   # also with zero frames
        for j, w in enumerate(want):
            assert torch.equal(torch.cat([p[j] for p in parts], 1), w), (T, j)


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    EINVAL, EUNSUPPORTED = -1, -3
    fake = 256   # never dereferenced

    def call(B=2, T=1000, F=5, M=22, Q=4, I=2, adaptive=1, pre=0.0, hop=240, W=960, x=fake, window=fake, gain=fake, a=fake):
        return lib.golf_lpc_source_filter_f32(x, T, window, gain, a, None, None, B, T, F, M, Q, I, adaptive, pre, hop, W,
                                              -(W // 2), 1e-9, 1e-12, None)

    for kw in (dict(x=None), dict(window=None), dict(gain=None), dict(a=None)):
        assert call(**kw) == EINVAL and b"lpc_source_filter" in lib.golf_last_error() and b"null" in lib.golf_last_error()
    for pre in (1.0, -1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(adaptive=0, pre=pre) == EINVAL and b"preemphasis" in lib.golf_last_error()
    assert call(adaptive=1, pre=float("nan"), x=None) == EINVAL and b"null" in lib.golf_last_error()   # unused when adaptive
    assert call(M=0) == EUNSUPPORTED and call(M=65) == EUNSUPPORTED and b"order" in lib.golf_last_error()
    assert call(Q=0) == EUNSUPPORTED and call(Q=17) == EUNSUPPORTED and b"source order" in lib.golf_last_error()
    assert call(I=-1) == EUNSUPPORTED and call(I=9) == EUNSUPPORTED and b"iterations" in lib.golf_last_error()
    assert call(W=26) == EUNSUPPORTED and b"M + Q" in lib.golf_last_error()
    assert call(W=22) == EUNSUPPORTED
    assert call(W=4097) == EUNSUPPORTED and b"LDS" in lib.golf_last_error()
    assert call(hop=0) == EUNSUPPORTED and b"hop" in lib.golf_last_error()
    assert call(B=1 << 16, F=1 << 15) == EUNSUPPORTED and b"2^31" in lib.golf_last_error()
    assert call(F=0) == EINVAL and call(B=-1) == EINVAL and call(T=-1) == EINVAL
    # an empty batch is no error, with the pointers an empty tensor has; its arguments are still checked
    assert call(B=0, x=None, gain=None, a=None) == 0
    assert call(B=0, Q=17) == EUNSUPPORTED and call(B=0, adaptive=0, pre=1.0) == EINVAL
