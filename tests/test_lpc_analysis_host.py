"""CPU: the host side of the LPC analysis -- the float64 restatement (tests/lpc_analysis_ref.py) against the numpy analysis
that produced tests/golden/g25 (oracle/make_lpc_tracks.py), frame conventions, the logits of LPCAnalysis against the
control transform they invert, and the C entries' argument checks without a GPU."""
import numpy as np
import pytest
import torch

import lpc_analysis_ref as R


def test_restatement_reproduces_make_lpc_tracks(golden):
    """centred=False, W=960, hop=240, M=22, periodic Hann in float64: a to 1e-9 abs, gain * sqrt(sum w^2 / W) to 1e-9 abs
    (measured 1.4e-11 and 1.7e-13 when this was written)."""
    from oracle import make_lpc_tracks as MK

    x = R.speech_like(golden, (0, 9), 4801)
    w = np.hanning(MK.WIN + 1)[:-1]
    for row in x:
        A, G = MK.analyse(row)
        gain, a, rc = R.analysis(row[None], w, MK.HOP, MK.ORDER, centred=False)
        assert a.shape == (1,) + A.shape and gain.shape == (1,) + G.shape
        ea = np.abs(a[0].numpy() - A).max()
        eg = np.abs(gain[0].numpy() * np.sqrt((w * w).sum() / MK.WIN) - G).max()
        print(f"a {ea:.2e}  gain {eg:.2e}  max |rc| {rc.abs().max():.4f}")
        assert ea <= 1e-9 and eg <= 1e-9


@pytest.mark.parametrize("T,W,hop,centred,n_frames,F", [
    (1000, 960, 240, True, None, 5), (1000, 960, 240, False, None, 1), (4801, 960, 240, False, None, 17),
    (100, 256, 64, True, None, 2), (100, 256, 64, False, None, 1),        # T < W
    (300, 128, 200, True, None, 2), (600, 128, 200, False, None, 3),      # hop > W
    (777, 51, 7, True, None, 112), (777, 50, 7, True, 120, 120), (1000, 960, 240, True, 3, 3)])
def test_frames(T, W, hop, centred, n_frames, F):
    from golf_amd.functional import lpc_analysis_frames

    x = torch.arange(1, T + 1, dtype=torch.float64)[None]
    fr = R.frames(x, W, hop, centred, n_frames)[0]
    assert fr.shape == (F, W)
    if n_frames is None:
        assert lpc_analysis_frames(T, W, hop, centred) == F
    o = -(W // 2) if centred else 0
    for f in sorted({0, 1 % F, F // 2, F - 1}):           # first, edge and last frames, every tap
        t = o + f * hop + np.arange(W)
        want = np.where((t >= 0) & (t < T), t + 1, 0)
        assert np.array_equal(fr[f].numpy(), want), f


def test_rc2lpc_of_rc_is_a_and_silence():
    from oracle import golf_oracle as O

    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (3, 900))
    x[1, 200:700] = 0.0
    x[2] = 0.0
    w = np.hanning(129)[:-1]
    gain, a, rc = R.analysis(x, w, 32, 13)
    assert np.abs(O.rc2lpc(rc.numpy()) - a.numpy()).max() <= 1e-12
    assert rc.abs().max() < 1.0
    # all-zero signal: a = 0, gain = sqrt(eps_abs / sum w^2); the same on the silent frames of row 1
    silent = np.sqrt(1e-12 / (w * w).sum())
    assert torch.all(a[2] == 0) and torch.all(rc[2] == 0) and np.allclose(gain[2].numpy(), silent, rtol=1e-12, atol=0)
    fr = R.frames(torch.tensor(x), 128, 32)[1]
    quiet = (fr.abs().amax(-1) == 0).numpy()
    assert quiet.sum() >= 10
    assert torch.all(a[1][quiet] == 0) and np.allclose(gain[1].numpy()[quiet], silent, rtol=1e-12, atol=0)
    assert np.all(np.abs(a[1].numpy()[~quiet]).max(-1) > 0)


def test_logits_invert_the_control_transform():
    """to_logits of (gain, rc) from the restatement, through LTVMinimumPhaseFilterPrecise's control transform, is (gain, a)
    again: 1e-5 rel-max on a case with |rc| <= 0.99."""
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise
    from golf_amd.lpc import LPCAnalysis

    M, hop = 10, 64
    rng = np.random.default_rng(5)
    ex = rng.normal(0, 1, (2, 2000))
    x = np.zeros_like(ex)
    for t in range(2000):   # a mild two-pole colouring
        x[:, t] = ex[:, t] + 1.2 * x[:, t - 1] - 0.6 * x[:, t - 2]
    gain, a, rc = R.analysis(x, torch.hann_window(256, dtype=torch.float64), hop, M)
    assert 0.3 < rc.abs().max() <= 0.99
    for mx in (1.0, 0.995):
        log_gain, logits = LPCAnalysis.to_logits(gain.float(), rc.float(), mx)
        assert log_gain.shape == (2, gain.shape[1], 1) and logits.shape == rc.shape
        filt = LTVMinimumPhaseFilterPrecise(lpc_order=M, max_abs_value=mx)
        assert filt.ctrl.split_size == (1, M)
        g2, a2 = filt.ctrl.trsfm_fn(AudioTensor(log_gain, hop), AudioTensor(logits, hop))
        eg = (g2.as_tensor()[..., 0].double() - gain).abs().max() / gain.abs().max()
        ea = (a2.as_tensor().double() - a).abs().max() / a.abs().max()
        print(f"max_abs_value {mx}: gain {eg:.2e}  a {ea:.2e}")
        assert eg <= 1e-5 and ea <= 1e-5


def test_module_surface():
    from golf_amd import lpc
    from golf_amd.lpc import LPCAnalysis

    assert "LPCAnalysis" in lpc.__all__
    m = LPCAnalysis(22, 240)
    assert m.window_length == 960 and m._window.shape == (960,) and m._window.dtype == torch.float32
    assert not m.state_dict() and m.centred
    assert LPCAnalysis(8, 100, window_length=256, window="hanning", centred=False)._window.shape == (256,)
    from golf_amd._lib import GolfError

    with pytest.raises(GolfError, match="no CPU path"):
        m(torch.zeros(1, 1000))


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "lpc_analysis.hip" in _lib.SOURCES and lib.golf_abi_version() == _lib.ABI_VERSION == 6
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
    assert lib.golf_lpc_analysis_workspace_bytes(2, 21, 22) == 7936    # 2 * 21 * 23 doubles = 7728 bytes, rounded up to 256
    assert lib.golf_lpc_analysis_workspace_bytes(32, 201, 22) == 32 * 201 * 23 * 8
    assert lib.golf_lpc_analysis_workspace_bytes(0, 21, 22) == 0 and lib.golf_lpc_analysis_workspace_bytes(2, 21, 65) == 0
    fake = 256   # never dereferenced
    big = 1 << 40

    def fwd(B=2, T=1000, F=5, M=22, hop=240, W=960, x=fake, ws=fake, nbytes=big):
        return lib.golf_lpc_analysis_fwd_f32(x, T, fake, fake, fake, fake, ws, nbytes, B, T, F, M, hop, W, -(W // 2), 1e-9,
                                             1e-12, None)

    def bwd(B=2, T=1000, F=5, M=22, hop=240, W=960, lags=fake, ws=fake, nbytes=big):
        return lib.golf_lpc_analysis_bwd_f32(fake, fake, fake, fake, T, fake, lags, fake, T, ws, nbytes, B, T, F, M, hop, W,
                                             -(W // 2), 1e-9, None)

    for call, name in ((fwd, b"lpc_analysis_fwd"), (bwd, b"lpc_analysis_bwd")):
        assert call(ws=None) == EINVAL and name in lib.golf_last_error() and b"null" in lib.golf_last_error()
        assert call(M=0) == EUNSUPPORTED and call(M=65) == EUNSUPPORTED and b"order" in lib.golf_last_error()
        assert call(M=22, W=22) == EUNSUPPORTED and b"exceed the order" in lib.golf_last_error()
        assert call(W=4097) == EUNSUPPORTED and b"LDS" in lib.golf_last_error()
        assert call(hop=0) == EUNSUPPORTED and b"hop" in lib.golf_last_error()
        assert call(B=1 << 16, F=1 << 15) == EUNSUPPORTED and b"2^31" in lib.golf_last_error()
        assert call(nbytes=16) == EWORKSPACE and call(ws=8) == EWORKSPACE
        assert call(B=0) == EINVAL
    assert fwd(x=None) == EINVAL and bwd(lags=None) == EINVAL
