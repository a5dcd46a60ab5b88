"""CPU: the host side of the harmonic-plus-noise analysis -- the float64 restatement (tests/hna_ref.py) on signals built as
the oscillator bank builds them, its fp32 stand-in held to the bars of the GPU test on the GPU test's inputs, the refusals of
golf_harmonic_analysis_f32 (none launches) and the Python surface without a device."""
import numpy as np
import pytest
import torch

import hna_ref as R

TOL = 1e-4        # the GPU test's parity bar, in units of the frame's scale
ESTIMATOR = 1e-3  # recovery of planted amplitudes on gliding f0, in units of the largest amplitude
SIGMA = 0.05
F, K = 101, 40    # 1 s at 24 kHz, hop 240


def planted(kind, noise=0.0, seed=0):
    """(x float64, f0 fp32, amplitudes (F, K) = 0.5 / k, interior frames): the bank's signal on the track ``kind``."""
    f0 = R.track(kind, F)
    amps = np.tile(0.5 / np.arange(1, K + 1), (F, 1))
    x = R.bank(f0.astype(np.float64), amps, R.HOP, R.SR)
    if noise:
        x = x + noise * np.random.default_rng(seed).normal(0, 1, len(x))
    return x, f0, amps


def interior(out, T):
    L = out["L"][0]
    return [f for f in range(len(L)) if f * R.HOP - L[f] // 2 >= 0 and f * R.HOP - L[f] // 2 + L[f] <= T]


@pytest.mark.parametrize("kind,bar", [("const200", 1e-9), ("const173", 1e-4), ("glide150", ESTIMATOR), ("glide80", ESTIMATOR),
                                      ("vibrato", ESTIMATOR)])
def test_reference_recovers_planted_amplitudes(kind, bar):
    x, f0, amps = planted(kind)
    out = R.analyse(x[None], f0[None], R.SR, R.HOP, K)
    inner = interior(out, len(x))
    err = np.abs(out["amp"][0, inner] - amps[inner]).max() / 0.5
    print(f"{kind}: {len(inner)} interior frames, worst amplitude error {err:.2e} of the largest amplitude")
    assert len(inner) >= 90 and out["voiced"].all()
    assert err <= bar


@pytest.mark.parametrize("kind", ["const200", "glide150", "vibrato"])
def test_reference_noise_level(kind):
    x, f0, _ = planted(kind, noise=SIGMA, seed=7)
    out = R.analyse(x[None], f0[None], R.SR, R.HOP, K, n_mag=65, smooth=4)
    inner = interior(out, len(x))
    level = np.sqrt(np.exp(2 * out["log_mag"][0, inner]).mean())
    print(f"{kind}: noise level {level / SIGMA:.3f} sigma")
    assert 0.7 * SIGMA <= level <= 1.05 * SIGMA


def test_reference_unvoiced_frames():
    """Amplitudes and phases exactly 0, and the noise spectrum is that of x itself under the window."""
    rng = np.random.default_rng(3)
    x = rng.normal(0, 0.1, 2401)
    f0 = np.zeros((1, 11), np.float32)
    out = R.analyse(x[None], f0, R.SR, R.HOP, 20, n_mag=33)
    assert (out["amp"] == 0).all() and (out["phase"] == 0).all() and (out["L"] == 4 * R.HOP).all()
    L, f = 4 * R.HOP, 5
    i = np.arange(L)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * (i + 0.5) / L)
    seg = x[f * R.HOP - L // 2: f * R.HOP - L // 2 + L]
    m = i - L // 2
    for b in (0, 7, 32):
        S = abs(np.sum(w * seg * np.exp(-1j * np.pi * b * m / 32))) ** 2 / np.sum(w * w)
        assert abs(out["log_mag"][0, f, b] - 0.5 * np.log(S + 1e-12)) <= 1e-9
    # white noise of variance v: E S_b = v
    level = np.sqrt(np.exp(2 * out["log_mag"][0, 2:9]).mean())
    assert 0.8 * 0.1 <= level <= 1.2 * 0.1


def test_reference_mutes_at_nyquist():
    f0 = np.full((1, 5), 1000.0, np.float32)
    x = R.voice(np.full(5, 1000.0), 960, 11, 1)
    out = R.analyse(x[None], f0, R.SR, R.HOP, 16, n_mag=0)
    assert (out["amp"][..., 11:] == 0).all() and (out["amp"][0, 2, :11] > 0).all()
    assert (out["L"] == 480).all()                     # n_per raised from 4 to 20 by min_window = 2 hop


def test_cases_reach_their_edges():
    c = R.cases()
    L = {n: R.reference(n)["L"] for n in ("L1600", "L_clamped", "L480_min_window", "L_odd", "unvoiced_odd", "unvoiced_limit")}
    assert (L["L1600"] == 1600).all() and (L["L_clamped"] == 2048).all() and (L["L480_min_window"] == 480).all()
    assert (L["L_odd"] == 961).all() and (L["unvoiced_odd"] == 2047).all() and (L["unvoiced_limit"] == 2048).all()
    rules = R.reference("K1")["rule"]
    assert list(rules[0]) == ["forward", "central", "backward", "unvoiced", "none", "unvoiced", "forward", "backward",
                              "unvoiced", "unvoiced", "none"]
    assert rules[1][0] == "unvoiced" and rules[1][2] == "forward" and rules[1][5] == "backward" and rules[1][10] == "backward"
    assert set(rules[1]) >= {"central"}
    x, f0, kw = c["T_lt_window"]
    assert x.shape[1] < R.reference("T_lt_window")["L"].min()
    assert c["F1"][1].shape == (1, 1)
    x, f0, kw = c["more_frames"]
    ref = R.reference("more_frames")
    assert f0.shape[1] > x.shape[1] // kw["hop"] + 1 and (ref["scale"][0, 8:] == 0).all() and (ref["amp"][0, 8:] == 0).all()
    assert all(v[0].shape[0] <= 3 and v[0].shape[1] <= 4800 for n, v in c.items() if n != "recipe")
    assert c["recipe"][0].shape == (4, 4801) and c["recipe"][2]["K"] == 155 and c["recipe"][2]["n_mag"] == 256
    steep = c["steep_glide"][1][0]
    assert abs(steep[20] / steep[0] - 2 ** 0.8) < 1e-6   # 0.2 s: 0.8 of an octave


@pytest.mark.parametrize("name", list(R.cases()))
def test_fp32_stand_in_meets_the_gpu_bars(name):
    """The evidence that the GPU test's bars leave room for a correct fp32 kernel."""
    x, f0, kw = R.cases()[name]
    ref, low = R.reference(name), R.analyse(x, f0, fp32=True, **kw)
    e_amp, e_mag, e_ph = R.errors(low, ref)
    print(f"{name}: amp {e_amp:.2e}  mag {e_mag:.2e}  phase {e_ph:.2e}  (units of the frame's scale)")
    assert e_amp <= TOL and e_mag <= TOL and e_ph <= TOL
    assert (low["amp"][ref["amp"] == 0] == 0).all()


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "harm_analysis.hip" in _lib.SOURCES and lib.golf_abi_version() == _lib.ABI_VERSION == 6
    EINVAL = -1
    fake = 256   # never dereferenced

    def call(x=fake, xs=None, f0=fake, fs=None, amp=fake, phases=fake, log_mag=fake, B=2, T=1000, F=5, K=20, n_mag=65,
             hop=240, periods=4, min_window=480, max_window=2048, unvoiced_window=960, smooth=0, sr=24000.0, eps=1e-12):
        rc = lib.golf_harmonic_analysis_f32(x, T if xs is None else xs, f0, F if fs is None else fs, amp, phases, log_mag, B,
                                            T, F, K, n_mag, hop, periods, min_window, max_window, unvoiced_window, smooth,
                                            sr, eps, None)
        if rc:
            assert b"harmonic_analysis" in lib.golf_last_error()
        return rc

    for kw, word in ((dict(x=None), b"null"), (dict(f0=None), b"null"), (dict(amp=None), b"null"), (dict(B=0), b"size"),
                     (dict(T=-1), b"size"), (dict(F=0), b"size"), (dict(xs=999), b"stride"), (dict(fs=4), b"stride"),
                     (dict(K=0), b"harmonics"), (dict(K=257), b"harmonics"), (dict(n_mag=1), b"n_mag"),
                     (dict(n_mag=-1), b"n_mag"), (dict(n_mag=514), b"n_mag"), (dict(hop=0), b"hop"),
                     (dict(periods=1), b"periods"), (dict(min_window=2049), b"min_window"),
                     (dict(min_window=600, max_window=512), b"min_window"), (dict(min_window=0), b"min_window"),
                     (dict(max_window=2049), b"max_window"), (dict(max_window=1, min_window=1), b"max_window"),
                     (dict(unvoiced_window=2049), b"unvoiced_window"), (dict(unvoiced_window=1), b"unvoiced_window"),
                     (dict(smooth=65), b"smooth"), (dict(smooth=-1), b"smooth"), (dict(sr=0.0), b"sample_rate"),
                     (dict(sr=float("nan")), b"sample_rate"), (dict(eps=-1.0), b"eps"),
                     (dict(B=1 << 16, F=1 << 15), b"2^31")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())


def test_python_surface_without_a_device():
    from golf_amd import functional as GF
    from golf_amd import hna
    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor

    assert "harmonic_analysis" in GF.__all__ and hna.__all__ == ["HarmonicNoiseAnalysis"]
    x, f0 = torch.zeros(2, 1000), torch.full((2, 5), 100.0)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.harmonic_analysis(x, f0, 24000, 240, 20, n_mag=65)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.harmonic_analysis(x[:0], f0[:0], 24000, 240, 20)
    with pytest.raises(GolfError, match="must be \\(B, T\\)"):
        GF.harmonic_analysis(torch.zeros(1000), f0, 24000, 240, 20)
    with pytest.raises(GolfError, match="f0 must be \\(B, F\\)"):
        GF.harmonic_analysis(x, f0[0], 24000, 240, 20)
    with pytest.raises(GolfError, match="f0 must be \\(B, F\\)"):
        GF.harmonic_analysis(x, f0[:1], 24000, 240, 20)
    for kw, what in ((dict(hop=0), "hop"), (dict(num_harmonics=257), "num_harmonics"), (dict(n_mag=1), "n_mag"),
                     (dict(n_mag=514), "n_mag"), (dict(periods=1), "periods"), (dict(max_window=4096), "max_window"),
                     (dict(min_window=4096), "min_window"), (dict(unvoiced_window=4096), "unvoiced_window"),
                     (dict(n_mag=65, smooth=65), "smooth"), (dict(sample_rate=0), "sample_rate"), (dict(eps=-1), "eps")):
        args = dict(dict(sample_rate=24000, hop=240, num_harmonics=20), **kw)
        with pytest.raises(GolfError, match=what):   # before any tensor is looked at: argument errors come first
            GF.harmonic_analysis(x, f0, **args)
    m = hna.HarmonicNoiseAnalysis(24000, 240, 155, n_mag=256)
    assert (m.min_window, m.unvoiced_window, m.max_window, m.periods, m.smooth, m.eps) == (480, 960, 2048, 4, 0, 1e-12)
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    for call in (m, m.analyse):
        with pytest.raises(GolfError, match="no CPU path"):
            call(x, f0)
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(x, 2), f0)
    with pytest.raises(AssertionError, match="hop 240"):
        m(x, AudioTensor(f0, 120))
