"""CPU: the host side of the spectral-envelope analysis -- the float64 restatement (tests/env_ref.py) on signals with a planted
envelope, its fp32 stand-in held to the bars of the GPU test on the GPU test's inputs, the refusals of
golf_spectral_envelope_f32 (none launches) and the Python surface without a device."""
import math

import numpy as np
import pytest
import torch

import env_ref as R

TOL = 1e-4          # the GPU test's bar on magnitudes, in units of the frame's largest magnitude
CEPS_TOL = 3e-6     # the GPU test's bar on ceps in nepers: 4 x the stand-in's worst error (test_fp32_stand_in_meets_the_gpu_bars)
MAX_DB, RMS_DB = 1.5, 0.3   # the estimator's own error on a planted envelope
F = 51              # 0.5 s at 24 kHz, hop 240
TRACKS = {"const100": np.full(F, 100.0), "const173": np.full(F, 173.3), "const400": np.full(F, 400.0),
          "glide150": np.linspace(150.0, 250.0, F)}
_planted = {}


def planted(kind):
    """(x float64, f0 fp32, the float64 analysis with every coefficient) of a track, computed once."""
    if kind not in _planted:
        f0 = TRACKS[kind].astype(np.float32)
        x = R.pulse_voice(f0.astype(np.float64), R.HOP, R.SR)
        _planted[kind] = (x, f0, R.analyse(x[None], f0[None], R.SR, R.HOP))
    return _planted[kind]


@pytest.mark.parametrize("kind", list(TRACKS))
def test_reference_recovers_planted_envelope(kind):
    """Measured here: const100 0.65 / 0.17 / -0.16 dB (max / rms / mean), const173 0.55 / 0.19, const400 1.36 / 0.18,
    glide150 0.94 / 0.17."""
    x, f0, out = planted(kind)
    worst, rms, mean = R.recovery_errors(out)
    print(f"{kind}: max {worst:.2f} dB  rms {rms:.2f} dB  mean {mean:.2f} dB")
    assert out["voiced"].all() and len(x) == 12001
    assert worst <= MAX_DB and rms <= RMS_DB


def test_reference_unit_convention():
    """Without the offset a pulse train through H measures as |H|^2 / 2: the mean error is -3.0 dB."""
    x, f0, _ = planted("const100")
    out = R.analyse(x[None], f0[None], R.SR, R.HOP, voiced_offset=0.0)
    mean = R.recovery_errors(out)[2]
    print(f"mean error without the offset {mean:.2f} dB")
    assert abs(mean + 3.0) <= 0.3


def test_reference_white_noise_level():
    sigma = 0.05
    x = np.random.default_rng(1).normal(0, sigma, 12001)
    out = R.analyse(x[None], np.zeros((1, F), np.float32), R.SR, R.HOP)
    level = math.sqrt(np.exp(2 * out["log_env"]).mean())
    print(f"white noise: level {level / sigma:.3f} sigma")
    assert not out["voiced"].any() and (out["fe"] == 500.0).all()
    assert 0.9 * sigma <= level <= 1.1 * sigma


def test_reference_steps_on_one_frame():
    """The transforms and the smoothing against their definitions written the long way, on one frame."""
    x, f0, _ = planted("const173")
    n, nh = R.N_FFT, R.N_FFT // 2
    f0_floor, f0_ceil = R.defaults(R.SR, n)
    voiced, fe, hw, r0, r = R.frame_constants(f0[20], R.SR, n, f0_floor, f0_ceil, 500.0)
    assert voiced and hw == math.floor(1.5 * R.SR / fe + 0.5) and abs(r - fe * n / R.SR / 3) < 1e-12
    seg = x[20 * R.HOP - hw: 20 * R.HOP + hw + 1]
    cl, P, Ps = R.analyse_frame(seg, fe, hw, r0, r, R.SR, n, -0.15, 1e-12)
    m = np.arange(-hw, hw + 1)
    w = 0.5 + 0.5 * np.cos(2 * np.pi * m * fe / (3 * R.SR))
    xw = w * seg
    xw = xw - w * xw.sum() / w.sum()
    for k in (0, 7, 300, nh):
        assert abs(abs(np.sum(xw * np.exp(-2j * np.pi * k * m / n))) ** 2 / np.sum(w * w) - P[k]) <= 1e-12 * P.max()
    # the smoothing as an integral of the piecewise-constant extension, by a fine Riemann sum
    Pc = P.copy()
    for k in range(nh + 1):
        if k < r0:
            u = r0 - k
            i0 = int(u)
            Pc[k] += (1 - (u - i0)) * P[i0] + (u - i0) * P[min(i0 + 1, nh)]
    ext = lambda j: Pc[abs(j) if abs(j) <= nh else 2 * nh - abs(j)]
    for k in (0, 1, 100, nh):
        ts = k - r + (np.arange(20000) + 0.5) * (2 * r / 20000)
        fine = np.mean([ext(int(math.floor(t + 0.5))) for t in ts])
        assert abs(fine - Ps[k]) <= 2e-4 * Ps[k]
    # the cepstrum is numpy's irfft of the log, liftered
    c = np.fft.irfft(np.log(Ps + 1e-12), n)[:nh + 1]
    q = np.arange(nh + 1)
    lift = np.sinc(fe * q / R.SR) * (1.3 - 0.3 * np.cos(2 * np.pi * fe * q / R.SR))
    assert np.abs(cl - c * lift).max() <= 1e-12


def test_smoothing_cell_edges():
    """r an integer, a half-integer and below 1/2: the covered fractions on a spectrum whose cells are known."""
    P = np.arange(9, dtype=np.float64) ** 2
    ext = lambda j: P[abs(j) if abs(j) <= 8 else 16 - abs(j)]
    for r in (2.0, 2.5, 1.0, 0.5, 0.25, 0.75):
        got = R.smooth(P, r)
        for k in range(9):
            lo, hi = k - r, k + r
            want = sum(max(0.0, min(hi, j + 0.5) - max(lo, j - 0.5)) * ext(j) for j in range(k - 4, k + 5)) / (2 * r)
            assert abs(got[k] - want) <= 1e-12 * max(want, 1.0), (r, k)
    assert np.allclose(R.smooth(P, 0.25), P) and R.smooth(P, 0.5)[3] == P[3]   # inside one cell
    assert abs(R.smooth(P, 1.0)[3] - (0.5 * P[2] + P[3] + 0.5 * P[4]) / 2) < 1e-12
    assert abs(R.smooth(P, 1.0)[0] - (P[0] + P[1]) / 2) < 1e-12              # the even extension about bin 0
    assert abs(R.smooth(P, 1.0)[8] - (P[8] + P[7]) / 2) < 1e-12              # and about bin n/2


def _cep_filter(order, phase="zero"):
    from golf_amd.filters import LTVCepFilter

    return LTVCepFilter(order, R.N_FFT, "hanning", R.HOP, phase=phase).double()


def test_ceps_is_the_cep_filters_control():
    """With every coefficient LTVCepFilter's response is exp(log_env) to rounding; at order 240 the truncation costs at most
    0.1 dB (measured 0.066 dB)."""
    _, _, out = planted("glide150")
    nb = R.N_FFT // 2 + 1
    ceps, env = torch.from_numpy(out["ceps"]), np.exp(out["log_env"])
    H = _cep_filter(nb - 1).frequency_response(ceps)[:, :nb].transpose(1, 2).numpy()
    assert np.abs(H / env - 1).max() <= 1e-10
    H = _cep_filter(240).frequency_response(ceps[..., :241])[:, :nb].transpose(1, 2).numpy()
    cut = R.DB * np.abs(np.log(H) - out["log_env"]).max()
    print(f"order 240 of 512: truncation {cut:.3f} dB")
    assert cut <= 0.1


def test_copy_synthesis_returns_the_envelope():
    """The pulse train of AdditivePulseTrain (its float64 restatement: the oscillator bank has no CPU path) through
    LTVCepFilter's stock path with the analysed ceps, analysed again, gives the first analysis's log_env on interior
    frames within the estimator's own bar."""
    from golf_amd.audiotensor import AudioTensor

    x, f0, out = planted("glide150")
    pulses = R.pulse_voice(f0.astype(np.float64), R.HOP, R.SR, ceps=np.zeros(1), noise=0.0)
    filt = _cep_filter(240, "min")
    y = filt(AudioTensor(torch.from_numpy(pulses)[None]), AudioTensor(torch.from_numpy(out["ceps"][..., :241]), R.HOP))
    y = y.as_tensor().numpy()
    again = R.analyse(y, f0[None], R.SR, R.HOP)
    d = R.DB * np.abs(again["log_env"][0, 5:-5, :487] - out["log_env"][0, 5:-5, :487])
    print(f"copy-synthesis: worst {d.max():.2f} dB, rms {math.sqrt((d * d).mean()):.2f} dB over interior frames")
    assert y.shape == (1, 12000) and d.max() <= MAX_DB


def test_cases_reach_their_edges():
    c = R.cases()
    assert all(v[0].shape[0] == 3 and 8 <= v[1].shape[1] <= 12 for v in c.values())
    assert {v[2]["n_fft"] for v in c.values()} == {64, 128, 256, 512, 1024, 2048} and c["n64"][2]["hop"] == 8
    assert c["n1024"][2]["hop"] == 240 and c["n1024"][2]["sample_rate"] == 24000.0
    ref = R.reference("clamps")
    assert (ref["hw"][0] == 511).all() and (ref["fe"][0] > 50.0).all()           # below the floor: 2 hw + 1 = n_fft - 1
    assert (ref["fe"][1] == 2000.0).all() and (ref["hw"][1] == 18).all()         # above the ceiling: the shortest window
    assert (R.reference("floor_1021")["hw"][0] == 510).all()                     # 2 hw + 1 = n_fft - 3
    ref = R.reference("cell_edges")
    assert (ref["r"][0] == 2.0).all() and (ref["r"][1] == 2.5).all() and (ref["r"][2] == 3.0).all()
    ref = R.reference("mixed")
    f0 = c["mixed"][1]
    assert np.isnan(f0).sum() == 3 and (f0 < 0).sum() == 2 and (f0 == 0).sum() >= 16
    assert (ref["voiced"] == (f0 > 0)).all() and (ref["fe"][~ref["voiced"]] == 500.0).all()
    assert c["T_short"][0].shape[1] == 150 < 2 * R.reference("T_short")["hw"].min() + 1
    assert c["T0"][0].shape == (3, 0)
    assert np.allclose(R.reference("T0")["log_env"] - np.where(R.reference("T0")["voiced"], R.OFFSET, 0)[..., None],
                       0.5 * math.log(1e-12), rtol=1e-12)
    assert R.reference("n_ceps1")["ceps"].shape[-1] == 1 and R.reference("n_ceps241")["ceps"].shape[-1] == 241
    # the smallest r any input can reach is 1 bin: three periods must fit the transform, so r0 = fe n / sr >= 3
    assert min(R.reference(n)["r"].min() for n in c) >= 1.0
    # every input carries noise 60 dB below its rms: no bin is numerically empty
    for name, (x, f0, kw) in c.items():
        if x.shape[1] > 1000:
            ref = R.reference(name)
            span = ref["log_env"].max(-1) - ref["log_env"].min(-1)
            assert span.max() <= 0.5 * math.log(1e6) + 6.0, (name, span.max())


@pytest.mark.parametrize("name", list(R.cases()))
def test_fp32_stand_in_meets_the_gpu_bars(name):
    """The evidence that the GPU test's bars leave room for a correct fp32 kernel.  The stand-in's worst ceps error over the
    cases is 5.3e-7 Np (mixed); 4 x that, rounded up to one digit, is the GPU test's 3e-6."""
    x, f0, kw = R.cases()[name]
    ref, low = R.reference(name), R.analyse(x, f0, fp32=True, **kw)
    e_env, e_ceps = R.errors(low, ref)
    print(f"{name}: magnitudes {e_env:.2e} of the frame's largest, ceps {e_ceps:.2e} Np")
    assert e_env <= TOL and e_ceps <= CEPS_TOL / 4


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "spec_envelope.hip" in _lib.SOURCES and lib.golf_abi_version() == _lib.ABI_VERSION == 6
    EINVAL, EUNSUPPORTED = -1, -3
    fake = 256   # never dereferenced

    def call(x=fake, xs=None, f0=fake, fs=None, log_env=fake, ceps=fake, B=2, T=1000, F=5, n_fft=1024, n_ceps=241, hop=240,
             sr=24000.0, f0_floor=71.0, f0_ceil=2000.0, unvoiced_f0=500.0, q1=-0.15, eps=1e-12, off=0.3):
        rc = lib.golf_spectral_envelope_f32(x, T if xs is None else xs, f0, F if fs is None else fs, log_env, ceps, B, T, F,
                                            n_fft, n_ceps, hop, sr, f0_floor, f0_ceil, unvoiced_f0, q1, eps, off, None)
        if rc:
            assert b"spectral_envelope" in lib.golf_last_error()
        return rc

    for kw, word in ((dict(B=0), b"size"), (dict(T=-1), b"size"), (dict(F=0), b"size"), (dict(f0=None), b"null"),
                     (dict(x=None), b"null"), (dict(log_env=None, ceps=None), b"both NULL"), (dict(n_ceps=0), b"n_ceps"),
                     (dict(xs=999), b"stride"), (dict(fs=4), b"stride"), (dict(hop=0), b"hop"), (dict(sr=0.0), b"sample_rate"),
                     (dict(sr=float("nan")), b"sample_rate"), (dict(eps=0.0), b"eps"), (dict(eps=-1.0), b"eps"),
                     (dict(n_ceps=-1, ceps=None), b"n_ceps"), (dict(n_ceps=514), b"n_ceps"), (dict(f0_floor=0.0), b"f0_floor"),
                     (dict(f0_floor=-5.0), b"f0_floor"), (dict(f0_floor=3000.0), b"f0_floor"),
                     (dict(f0_ceil=6001.0), b"f0_ceil"), (dict(unvoiced_f0=70.0), b"unvoiced_f0"),
                     (dict(unvoiced_f0=2001.0), b"unvoiced_f0"), (dict(unvoiced_f0=float("nan")), b"unvoiced_f0"),
                     (dict(f0_floor=70.0), b"longest window"), (dict(n_fft=512), b"longest window"),
                     (dict(B=1 << 16, F=1 << 15), b"2^31")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())
    for n in (32, 4096, 1000, 0, -1024):
        assert call(n_fft=n) == EUNSUPPORTED and b"n_fft" in lib.golf_last_error()
    # the edges the entry takes are not refused for their values: T = 0 without x, one output, the default floor.  These
    # would launch, so only the checks before them are run here: a refusal that comes last (B*F) proves the others passed
    for kw in (dict(T=0, x=None), dict(ceps=None, n_ceps=0), dict(log_env=None), dict(f0_floor=3 * 24000.0 / 1021),
               dict(f0_ceil=6000.0), dict(n_ceps=513)):
        assert call(B=1 << 16, F=1 << 15, **kw) == EINVAL and b"2^31" in lib.golf_last_error(), kw


def test_python_surface_without_a_device():
    from golf_amd import envelope
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor

    assert "spectral_envelope" in GF.__all__ and envelope.__all__ == ["SpectralEnvelopeAnalysis"]
    lo, hi = GF.spectral_envelope_defaults(24000.0, 1024)
    assert abs(lo - 70.519) < 1e-3 and hi == 2000.0 and (lo, hi) == R.defaults(24000.0, 1024)
    assert abs(GF.ENV_VOICED_OFFSET - 0.5 * math.log(2)) < 1e-15
    x, f0 = torch.zeros(2, 1000), torch.full((2, 5), 100.0)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.spectral_envelope(x, f0, 24000, 240)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.spectral_envelope(x[:0], f0[:0], 24000, 240, n_ceps=241)
    with pytest.raises(GolfError, match="must be \\(B, T\\)"):
        GF.spectral_envelope(torch.zeros(1000), f0, 24000, 240)
    with pytest.raises(GolfError, match="f0 must be \\(B, F\\)"):
        GF.spectral_envelope(x, f0[0], 24000, 240)
    with pytest.raises(GolfError, match="f0 must be \\(B, F\\)"):
        GF.spectral_envelope(x, f0[:1], 24000, 240)
    with pytest.raises(GolfError, match="frames"):
        GF.spectral_envelope(x, f0[:, :0], 24000, 240)
    for kw, what in ((dict(hop=0), "hop"), (dict(sample_rate=0), "sample_rate"), (dict(n_fft=1000), "n_fft"),
                     (dict(n_fft=32), "n_fft"), (dict(n_fft=4096), "n_fft"), (dict(n_ceps=514), "n_ceps"),
                     (dict(n_ceps=-1), "n_ceps"), (dict(return_log_env=False), "nothing to return"),
                     (dict(f0_floor=0), "f0_floor"), (dict(f0_floor=3000), "f0_floor"), (dict(f0_ceil=6001), "f0_ceil"),
                     (dict(unvoiced_f0=60), "unvoiced_f0"), (dict(unvoiced_f0=2500), "unvoiced_f0"),
                     (dict(f0_floor=70), "longest window"), (dict(n_fft=512, f0_floor=71), "longest window"), (dict(eps=0), "eps"),
                     (dict(q1=float("nan")), "q1")):
        args = dict(dict(sample_rate=24000, hop=240), **kw)
        with pytest.raises(GolfError, match=what):   # before any tensor is looked at: argument errors come first
            GF.spectral_envelope(x, f0, **args)
    m = envelope.SpectralEnvelopeAnalysis(24000, 240, filter_order=240)
    assert (m.n_fft, m.f0_floor, m.f0_ceil, m.unvoiced_f0, m.q1, m.eps) == (1024, lo, hi, 500.0, -0.15, 1e-12)
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    for call in (m, m.analyse, m.response_rows):
        with pytest.raises(GolfError, match="no CPU path"):
            call(x, f0)
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(x, 2), f0)
    with pytest.raises(AssertionError, match="hop 240"):
        m(x, AudioTensor(f0, 120))
