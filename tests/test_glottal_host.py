"""CPU: the float64 restatement of the glottal-source match (tests/glottal_ref.py) against band-limited pulses with a planted
table position, the plan builder against direct float64 sums, the fp32 stand-in against the GPU test's bars, the refusals of
golf_glottal_match_f32 (none launches) and the Python surface without a device.

Measured with the package's 100 x 1000 table, 64 harmonics, 256 shifts, the glide 110-180 Hz with vibrato, a random-walk w
and 1 % white noise (profiles/glottal_parity.txt): w within 1.12 table steps (rms 0.66) on interior frames, 0.70 (0.44) for a
constant w = 0.3; theta within 1.4e-3 cycles; rho >= 0.9998 on voiced frames against <= 0.33 on white noise.  Each bar below
is the measured figure plus 25 %, the margin for the generator's seed."""
import numpy as np
import pytest
import torch

import glottal_ref as R

MARGIN = 1.25
RHO_TOL, THETA_TOL, W_TOL = 1.2e-7, 1.2e-7, 1.1e-4   # tests/test_gpu_glottal.py


def analysed(case, x=None):
    amp, ph = R.harmonics(case, x)
    return R.run(case, amp, ph)


def test_reference_recovers_a_planted_table_position():
    moving, const = R.planted_case("walk"), R.planted_case("const")
    w_max, w_rms, th = R.planted_errors(moving, analysed(moving))
    c_max, c_rms, c_th = R.planted_errors(const, analysed(const))
    print(f"random-walk w: max {w_max:.4f} rms {w_rms:.4f} steps, theta {th:.3e} cycles; constant w: max {c_max:.4f} rms "
          f"{c_rms:.4f} steps, theta {c_th:.3e} cycles")
    assert w_max <= MARGIN * R.PLANTED_W_MAX and w_rms <= MARGIN * R.PLANTED_W_RMS
    assert th <= MARGIN * R.PLANTED_THETA and c_th <= MARGIN * R.PLANTED_THETA
    assert c_max < w_max and c_rms < w_rms   # most of the error is w moving inside the four-period window


def test_reference_on_the_oscillators_rendition():
    """The reference of the GPU round trip: the same tracks as the oscillator renders them, in float64."""
    case = R.round_trip_case()
    w_max, w_rms, _ = R.planted_errors(case, analysed(case))
    print(f"oscillator's rendition: max {w_max:.4f} rms {w_rms:.4f} steps")
    assert R.ROUND_TRIP_W_MAX / 1.01 <= w_max <= 1.01 * R.ROUND_TRIP_W_MAX


def test_rho_separates_voiced_frames_from_noise():
    case = R.planted_case("walk")
    voiced = R.interior(analysed(case)["rho"])
    noise = analysed(case, np.random.default_rng(5).normal(0, 1, case["x"].shape).astype(np.float32))["rho"]
    print(f"rho: voiced >= {voiced.min():.4f}, white noise <= {noise.max():.4f} (mean {noise.mean():.4f})")
    assert noise.max() < R.RHO_BAR < voiced.min()
    assert abs(R.RHO_BAR - 0.5 * (0.33 + 0.999)) < 0.01   # midway between the two measured levels


def test_exact_harmonics_return_the_blend_exactly():
    """Harmonics that are a blend of two rows at a grid phase: step 6 inverts the blend, step 5 finds the column."""
    table = R.golf_table()
    S, N, X = R.plan(table, 32)
    Sc = S[..., 0].astype(np.float64) + 1j * S[..., 1]
    K, n_phi = table.shape[0], 128
    for w_true, j_true in ((0.0, 0), (1.0, 127), (0.3, 5), (29.5 / 99, 64), (0.7071, 77)):
        k0 = min(int(w_true * (K - 1)), K - 2)
        p = w_true * (K - 1) - k0
        c = ((1 - p) * Sc[k0] + p * Sc[k0 + 1]) * np.exp(2j * np.pi * np.arange(1, 33) * j_true / n_phi)
        amp = np.abs(c)[None, None].astype(np.float32)
        ph = np.mod(np.angle(c) / (2 * np.pi) + 0.25, 1.0)[None, None].astype(np.float32)
        for fp32 in (False, True):
            out = R.match(amp, ph, np.full((1, 1), 150.0, np.float32), S, N, X, R.SR, n_phi, fp32=fp32)
            dth = abs(out["theta"][0, 0] - j_true / n_phi)
            # (the parabola runs on the best single row, whose peak sits beside the blend's: exact for a pure row only)
            assert abs(out["w"][0, 0] - w_true) * (K - 1) <= 1e-3, (w_true, j_true, out)
            assert min(dth, 1 - dth) <= (1e-6 if p == 0 else 0.5 / n_phi), (w_true, j_true, out)
            assert abs(out["rho"][0, 0] - 1) <= 1e-6


def test_plan_builder():
    from golf_amd import functional as GF

    rng = np.random.default_rng(0)
    for K, L, H in ((5, 16, 12), (3, 15, 9), (100, 1000, 64), (2, 2, 1)):
        table = R.golf_table() if (K, L) == (100, 1000) else rng.normal(0, 1, (K, L)).astype(np.float32)
        plan = GF.glottal_plan(torch.tensor(table), H)
        S, N, X = (t.numpy() for t in (plan.spectrum, plan.norms, plan.cross))
        assert S.shape == (K, H, 2) and N.shape == (K, H) and X.shape == (K - 1, H)
        assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad
                   for t in (plan.spectrum, plan.norms, plan.cross))
        # the spectrum by its definition: a direct float64 sum over the table's points
        n = np.arange(L)
        direct = np.array([[2.0 / L * np.sum(table[k].astype(np.float64) * np.exp(-2j * np.pi * h * n / L)) if h <= L // 2
                            else 0.0 for h in range(1, H + 1)] for k in range(min(K, 5))])
        scale = np.abs(direct).max()
        assert np.abs(S[:5, :, 0] + 1j * S[:5, :, 1] - direct).max() <= 2e-7 * scale
        assert (S[:, L // 2:] == 0).all()   # harmonics above L/2
        # the prefix sums of the stored spectrum, direct float64 sums rounded once
        Sd = S.astype(np.float64)
        for h in range(H):
            want_n = (Sd[:, :h + 1] ** 2).sum((1, 2))
            want_x = (Sd[:-1, :h + 1] * Sd[1:, :h + 1]).sum((1, 2))
            assert np.abs(N[:, h] - want_n).max() <= 6e-8 * want_n.max() + 1e-45
            assert np.abs(X[:, h] - want_x).max() <= 6e-8 * np.abs(want_x).max() + 1e-45
        ours = R.plan(table, H)
        assert all(np.allclose(a, b, rtol=2e-7, atol=2e-7 * scale) for a, b in zip((S, N, X), ours))
    trainable = torch.nn.Parameter(torch.tensor(R.golf_table()))
    assert not GF.glottal_plan(trainable, 8).spectrum.requires_grad
    for bad, what in (((torch.zeros(1, 16), 4), "rows"), ((torch.zeros(1025, 4), 2), "rows"), ((torch.zeros(3, 1), 1), "points"),
                      ((torch.zeros(3, 16), 0), "num_harmonics"), ((torch.zeros(3, 16), 257), "num_harmonics"),
                      ((torch.zeros(16), 4), "must be \\(K, L\\)")):
        with pytest.raises(GF._lib.GolfError, match=what):
            GF.glottal_plan(*bad)


def test_cases_reach_their_edges():
    refs = {name: analysed(c) for name, c in R.cases().items() if name != "K1024"}
    assert (refs["H256_f400"]["Hf"] == 29).all()
    assert list(refs["nyquist"]["Hf"][0, [2, 3, 6]]) == [0, 0, 1] and np.isnan(refs["nyquist"]["w"][0, [2, 3]]).all()
    assert np.isnan(refs["zero_frame"]["w"]).sum() >= 1 and (refs["zero_frame"]["Hf"] == 8).all()   # E2 = 0, not Hf = 0
    K = R.cases()["edge_rows"]["table"].shape[0]
    assert (R.interior(refs["edge_rows"]["k"])[0] == 0).all() and (R.interior(refs["edge_rows"]["k"])[1] == K - 1).all()
    assert (R.interior(refs["edge_rows"]["w"])[0] < 0.5 / (K - 1)).all() and (R.interior(refs["edge_rows"]["w"])[1] > 1 - 0.5 / (K - 1)).all()
    j = R.interior(refs["wrap"]["j"])
    assert (j[0] == 0).all() and (j[1] == 63).all() and (j[2] == 0).all()
    assert np.isnan(refs["recipe"]["w"]).sum() == 3 and R.cases()["K1024"]["table"].shape[0] == 1024
    assert refs["smallest"]["w"].shape == (1, 9) and R.cases()["smallest"]["table"].shape[0] == 2
    for c in R.cases().values():
        assert c["x"].shape[0] <= 3 and c["f0"].shape[1] <= 40 and c["x"].shape[1] <= 9600


@pytest.mark.parametrize("name", list(R.cases()))
def test_fp32_stand_in_meets_the_gpu_bars(name):
    """The evidence that the GPU test's bars leave room for a correct kernel, and that the restatement finds no more than 2 %
    of a case's voiced frames tied.  The stand-in's largest errors over the cases are rho 2.9e-8, theta 3.0e-8 cycles and w
    2.8e-5 table steps (K1024): the rounding of the outputs to fp32; the GPU test's bars are four times those."""
    c = R.cases()[name]
    amp, ph = R.harmonics(c)
    ref, low = R.run(c, amp, ph), R.run(c, amp, ph, fp32=True)
    e_rho, e_theta, e_w, tied = R.errors(low, ref, c["table"].shape[0])
    print(f"{name}: rho {e_rho:.2e} theta {e_theta:.2e} cycles w {e_w:.2e} steps, {100 * tied:.1f} % tied")
    assert tied <= 0.02
    assert e_rho <= RHO_TOL / 4 * 1.05 and e_theta <= THETA_TOL / 4 * 1.05 and e_w <= W_TOL / 4 * 1.05


def test_argument_checks_without_gpu():
    """Every refusal comes before a launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    assert "glottal_match.hip" in _lib.SOURCES and lib.golf_abi_version() == _lib.ABI_VERSION == 6
    EINVAL, EUNSUPPORTED = -1, -3
    fake = 256   # never dereferenced

    def call(amp=fake, ph=fake, f0=fake, fs=None, S=fake, N=fake, X=fake, w=fake, theta=fake, rho=fake, B=2, F=5, H=64,
             K=100, n_phi=256, sr=24000.0):
        rc = lib.golf_glottal_match_f32(amp, ph, f0, F if fs is None else fs, S, N, X, w, theta, rho, B, F, H, K, n_phi, sr,
                                        None)
        if rc:
            assert b"glottal_match" in lib.golf_last_error()
        return rc

    for kw, word in ((dict(B=0), b"size"), (dict(F=0), b"size"), (dict(H=0), b"H="), (dict(H=257), b"H="), (dict(K=1), b"K="),
                     (dict(K=1025), b"K="), (dict(amp=None), b"null"), (dict(ph=None), b"null"), (dict(f0=None), b"null"),
                     (dict(S=None), b"plan"), (dict(N=None), b"plan"), (dict(X=None), b"plan"),
                     (dict(w=None, theta=None, rho=None), b"all NULL"), (dict(fs=4), b"stride"), (dict(sr=0.0), b"sample_rate"),
                     (dict(sr=-1.0), b"sample_rate"), (dict(sr=float("nan")), b"sample_rate"),
                     (dict(B=1 << 16, F=1 << 15), b"2^31")):
        assert call(**kw) == EINVAL, kw
        assert word in lib.golf_last_error(), (kw, lib.golf_last_error())
    for n in (4, 8192, 100, 0, -256):
        assert call(n_phi=n) == EUNSUPPORTED and b"n_phi" in lib.golf_last_error()
    # the edges the entry takes are not refused for their values.  These would launch, so only the checks before them are run
    # here: a refusal that comes last (B*F) proves the others passed
    for kw in (dict(H=1), dict(H=256), dict(K=2), dict(K=1024), dict(n_phi=8), dict(n_phi=4096), dict(w=None),
               dict(theta=None, rho=None), dict(w=None, rho=None)):
        assert call(B=1 << 16, F=1 << 15, **kw) == EINVAL and b"2^31" in lib.golf_last_error(), kw


def test_python_surface_without_a_device():
    import sys

    from golf_amd import functional as GF
    from golf_amd import glottal
    from golf_amd._lib import GolfError
    from golf_amd.audiotensor import AudioTensor
    from golf_amd.synth import GlottalFlowTable

    assert {"glottal_match", "glottal_plan", "GlottalPlan"} <= set(GF.__all__) and glottal.__all__ == ["GlottalSourceAnalysis"]
    assert "oracle" not in sys.modules or "oracle" not in open(glottal.__file__).read()
    table = torch.tensor(R.cases()["edge_rows"]["table"])
    plan = GF.glottal_plan(table, 8)
    amp, ph, f0 = torch.ones(2, 5, 8), torch.zeros(2, 5, 8), torch.full((2, 5), 100.0)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.glottal_match(amp, ph, f0, plan, 24000)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.glottal_match(amp[:0], ph[:0], f0[:0], plan, 24000)
    for args, what in (((amp[0], ph[0], f0, plan, 24000), "\\(B, F, H\\)"), ((amp, ph[:, :4], f0, plan, 24000), "\\(B, F, H\\)"),
                       ((amp, ph, f0[:1], plan, 24000), "f0 must be"), ((amp, ph, f0[0], plan, 24000), "f0 must be"),
                       ((amp, ph, f0, (plan.spectrum, plan.norms, plan.cross), 24000), "GlottalPlan"),
                       ((amp, ph, f0, GF.glottal_plan(table, 9), 24000), "harmonics"),
                       ((amp, ph, f0, GF.GlottalPlan(plan.spectrum, plan.norms[1:], plan.cross), 24000), "shapes"),
                       ((amp, ph, f0, GF.GlottalPlan(plan.spectrum, plan.norms.T.contiguous().T, plan.cross), 24000), "contiguous"),
                       ((amp, ph, f0, plan, 0), "sample_rate"), ((amp, ph, f0, plan, 24000, 100), "n_phi"),
                       ((amp, ph, f0, plan, 24000, 4), "n_phi"), ((amp, ph, f0, plan, 24000, 8192), "n_phi"),
                       ((amp[:, :0], ph[:, :0], f0[:, :0], plan, 24000), "frames")):
        with pytest.raises(GolfError, match=what):   # before any tensor is looked at: argument errors come first
            GF.glottal_match(*args)
    m = glottal.GlottalSourceAnalysis(table, 24000, 240, num_harmonics=8)
    assert (m.num_harmonics, m.n_phi, m.unvoiced_weight, m.periods, m.min_window, m.max_window) == (8, 256, 0.5, 4, 480, 2048)
    assert not list(m.parameters()) and not m.state_dict()   # the table and the plan are not persistent
    p1 = m.plan()
    assert torch.equal(p1.spectrum, plan.spectrum) and m.plan().spectrum.data_ptr() == p1.spectrum.data_ptr()
    osc = GlottalFlowTable(table_size=4, trainable=True)
    mo = glottal.GlottalSourceAnalysis(osc, 24000, 240, num_harmonics=8)
    assert [k for k in mo.state_dict()] == ["source.R_d_values", "source.table"] or "source.table" in mo.state_dict()
    first = mo.plan().spectrum.clone()
    with torch.no_grad():
        osc.table.mul_(2.0)   # in place: a new version, the same storage
    assert torch.allclose(mo.plan().spectrum, 2 * first, rtol=1e-6)
    x = torch.zeros(2, 1000)
    for call in (m, m.analyse, m.logits):
        with pytest.raises(GolfError, match="no CPU path"):
            call(x, f0)
    with pytest.raises(GolfError, match="no CPU path"):
        m.residual(x, torch.ones(2, 5), torch.zeros(2, 5, 4))
    with pytest.raises(AssertionError, match="hop 1"):
        m(AudioTensor(x, 2), f0)
    with pytest.raises(AssertionError, match="hop 240"):
        m(x, AudioTensor(f0, 120))
    with pytest.raises(TypeError):
        glottal.GlottalSourceAnalysis([[0.0, 1.0]], 24000, 240)
    with pytest.raises(GolfError, match="num_harmonics"):
        glottal.GlottalSourceAnalysis(table, 24000, 240, num_harmonics=300)
