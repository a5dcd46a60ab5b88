"""CPU: the host side of the f0 analysis -- the float64 restatement (tests/f0_ref.py) on signals of known f0, its fp32
stand-in held to the bars of the GPU test on the GPU test's inputs, the refusals of golf_f0_yin_f32 (none launches), the
frame count and the lag defaults, and the module without a device."""
import numpy as np
import pytest
import torch

import f0_ref as R

TOL = 1e-4


@pytest.fixture(scope="module")
def recipe():
    ref = R.reference("recipe")
    F = ref["f0"].shape[1]
    assert F == R.RECIPE["T"] // R.RECIPE["hop"] + 1 == 21
    return ref, slice(4, F - 4)   # frames 4 .. F-5: the interior frames


@pytest.mark.parametrize("row,f0", list(enumerate(R.RECIPE_TONES)))
def test_reference_finds_tones(recipe, row, f0):
    ref, inner = recipe
    est = ref["f0"][row, inner]
    print(f"{f0} Hz: worst relative error {np.abs(est / f0 - 1).max():.2e}, ap <= {ref['ap'][row, inner].max():.2e}")
    assert ref["voiced"][row, inner].all()
    assert np.abs(est / f0 - 1).max() <= 2e-3


def test_reference_on_noise_gap_noisy_tone_and_glide(recipe):
    ref, inner = recipe
    theta = R.RECIPE["threshold"]
    # white noise: nothing below the threshold anywhere
    assert not ref["voiced"][4].any() and not ref["found"][4].any() and (ref["f0"][4] == 0).all()
    assert ref["ap"][4].min() > theta
    # samples 1500 .. 3499 zeroed: the frames that lie wholly inside read only zeros
    hop, S = R.RECIPE["hop"], R.RECIPE["W"] + R.lags(R.RECIPE["sr"])[1]
    inside = [f for f in range(ref["f0"].shape[1]) if f * hop - S // 2 >= 1500 and f * hop - S // 2 + S <= 3500]
    assert inside == [10, 11]
    assert (ref["f0"][5, inside] == 0).all() and (ref["ap"][5, inside] == 1).all() and np.isfinite(ref["period"][5]).all()
    assert ref["voiced"][5, 4] and ref["voiced"][5, 16]
    # the 150.3 Hz tone in noise of power 0.09 against 0.77: voiced, so its ap is below the threshold by construction;
    # 1e-2 relative is a sixth of a semitone
    est = ref["f0"][6, inner]
    print(f"noisy tone: worst relative error {np.abs(est / 150.3 - 1).max():.2e}, ap <= {ref['ap'][6, inner].max():.2e}")
    assert ref["voiced"][6, inner].all() and ref["ap"][6, inner].max() < theta
    assert np.abs(est / 150.3 - 1).max() <= 1e-2
    # the glide against the instantaneous f0 at the frame's centre.  The samples a lag tau compares are centred (S - tau) / 2
    # <= tau_max / 2 = 200 samples before it: 40 Hz * 200 / 4801 = 1.7 Hz, 1.2 % of 140 Hz; 2 % with the estimate's own error
    fg = R.recipe_rows()[1]
    centre = np.arange(ref["f0"].shape[1])[inner] * hop
    err = np.abs(ref["f0"][7, inner] / fg[centre] - 1).max()
    print(f"glide: worst relative error {err:.2e}")
    assert ref["voiced"][7, inner].all() and err <= 2e-2


def test_search_branches_occur_in_the_reference():
    ref = R.reference("first_at_tau_min")
    assert (ref["first"] == 4).any()
    ref = R.reference("star_at_tau_max")
    at_end = ref["tau"] == 40
    assert at_end.any() and (ref["period"][at_end] == 40.0).all()           # no neighbour on the right: delta = 0
    ref = R.reference("walk")
    assert ((ref["tau"] - ref["first"] > 1) & ref["found"]).any()
    ref = R.reference("fallback")
    assert not ref["found"].any() and (ref["first"] == -1).all() and (ref["f0"] == 0).all()
    quiet, floored = R.reference("quiet"), R.reference("quiet_floor")
    assert quiet["voiced"].any() and not floored["voiced"].any() and (floored["f0"] == 0).all()
    assert np.array_equal(quiet["period"], floored["period"]) and np.array_equal(quiet["found"], floored["found"])
    ref = R.reference("more_frames")
    assert (ref["ap"][:, -4:] == 1).all() and (ref["f0"][:, -4:] == 0).all() and (ref["period"][:, -4:] == 4).all()


@pytest.mark.parametrize("name", list(R.cases()))
def test_fp32_stand_in_meets_the_gpu_bars(name):
    """The evidence that the GPU test's bars are reachable with an fp32 difference function: no frame changes its integer
    lag or its voicing, period within 1e-4 relative, ap within 1e-4 absolute."""
    x, kw = R.cases()[name]
    ref, low = R.reference(name), R.yin(x, fp32=True, **kw)
    flips = int(((ref["tau"] != low["tau"]) | (ref["voiced"] != low["voiced"])).sum())
    e_p = (np.abs(low["period"] - ref["period"]) / ref["period"]).max()
    e_ap = np.abs(low["ap"] - ref["ap"]).max()
    print(f"{name}: {ref['tau'].size} frames, {flips} differ; period {e_p:.2e}  ap {e_ap:.2e}  "
          f"d' {np.abs(low['dprime'] - ref['dprime']).max():.2e}")
    assert flips == 0 and e_p <= TOL and e_ap <= TOL


def test_frames_and_lag_defaults():
    from golf_amd import functional as GF

    for T, S, hop, centred, F in ((4801, 1424, 240, True, 21), (4801, 1424, 240, False, 15), (100, 296, 7, False, 1),
                                  (100, 296, 7, True, 15), (0, 90, 7, True, 1), (1424, 1424, 240, False, 1),
                                  (1664, 1424, 240, False, 2)):
        assert GF.f0_frames(T, S, hop, centred) == F == R.n_frames(T, S, hop, centred)
    assert GF.f0_lags(24000.0) == (24, 400, 800) == R.lags(24000.0)
    assert GF.f0_lags(24000.0, 60.0, 1000.0, 1024) == (24, 400, 1024)
    assert GF.f0_lags(44100.0, 80.0, 900.0) == (49, 552, 1104)            # floor(49.0), ceil(551.25)
    assert GF.f0_lags(8000.0, 200.0, 2000.0, 50) == (4, 40, 50)
    assert "f0_yin" in GF.__all__


def test_module_without_a_device():
    from golf_amd import f0
    from golf_amd._lib import GolfError
    from golf_amd.f0 import F0Analysis

    assert f0.__all__ == ["F0Analysis"]
    m = F0Analysis(24000, 240)
    assert (m.tau_min, m.tau_max, m.window_length) == (24, 400, 800) and m.centred and m.threshold == 0.15
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    assert F0Analysis(24000, 240, window_length=1024).window_length == 1024
    x = torch.zeros(1, 1000)
    for call in (m, m.analyse, m.voicing):
        with pytest.raises(GolfError, match="no CPU path"):
            call(x)
    from golf_amd import functional as GF

    with pytest.raises(GolfError, match="no CPU path"):
        GF.f0_yin(x, 24000, 240)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.f0_yin(torch.zeros(0, 1000), 24000, 240)
    for kw, what in ((dict(hop=0), "hop"), (dict(f0_max=30000.0), "lags"), (dict(f0_min=2000.0), "f0_min < f0_max"),
                     (dict(window_length=0), "window_length"), (dict(window_length=16000), "exceeds 16384"),
                     (dict(n_frames=0), "n_frames"), (dict(n_frames=2 ** 31), "2\\^31")):
        args = dict(dict(sample_rate=24000, hop=240), **kw)
        with pytest.raises(GolfError, match=what):   # before any tensor is looked at: argument errors come first
            GF.f0_yin(x, **args)
    with pytest.raises(GolfError, match="must be \\(B, T\\)"):
        GF.f0_yin(torch.zeros(1000), 24000, 240)


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "f0_yin.hip" in _lib.SOURCES and lib.golf_abi_version() == _lib.ABI_VERSION == 6
    EINVAL, EUNSUPPORTED = -1, -3
    fake = 256   # never dereferenced

    def call(x=fake, stride=None, f0=fake, period=fake, ap=fake, B=2, T=1000, F=5, hop=240, W=1024, tau_min=24, tau_max=400,
             sr=24000.0):
        return lib.golf_f0_yin_f32(x, T if stride is None else stride, f0, period, ap, B, T, F, hop, W, tau_min, tau_max,
                                   -((W + tau_max) // 2), sr, 0.15, 0.0, None)

    assert call(x=None) == EINVAL and b"f0_yin" in lib.golf_last_error() and b"null" in lib.golf_last_error()
    assert call(f0=None, period=None, ap=None) == EINVAL and b"at least one output" in lib.golf_last_error()
    assert call(B=0) == EINVAL and call(F=0) == EINVAL and call(T=-1) == EINVAL
    assert call(stride=999) == EINVAL and b"stride" in lib.golf_last_error()
    assert call(sr=0.0) == EINVAL and b"sample_rate" in lib.golf_last_error()
    assert call(hop=0) == EUNSUPPORTED and b"hop" in lib.golf_last_error()
    assert call(tau_min=0) == EUNSUPPORTED and b"tau_min" in lib.golf_last_error()
    assert call(tau_max=24) == EUNSUPPORTED and call(tau_max=10) == EUNSUPPORTED and b"exceed tau_min" in lib.golf_last_error()
    assert call(W=0) == EUNSUPPORTED and b"window" in lib.golf_last_error()
    assert call(W=16384 - 399) == EUNSUPPORTED and b"LDS" in lib.golf_last_error()        # S = 16385
    assert call(W=2 ** 31 - 1) == EUNSUPPORTED and b"LDS" in lib.golf_last_error()        # no overflow of W + tau_max
    assert call(B=1 << 16, F=1 << 15) == EUNSUPPORTED and b"2^31" in lib.golf_last_error()
