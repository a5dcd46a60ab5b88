"""CPU: the mel-cepstral filter LTVMLSAFilter2 -- class resolution and the config rewrite, the float64 module path against
the reference's own runs (g31), the numpy definition against the torch composition, the alpha = 0 identity with the cepstral
filter, the least-squares fit, and the argument checks of the C entries (refused before any launch: safe without a GPU)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import mlsa_ref
from conftest import GOLDEN


def _config():
    with open(os.path.join(GOLDEN, "g31_mlsa_config.json")) as f:
        return json.load(f)


def _end_filter_args(cfg):
    return cfg["model"]["init_args"]["decoder"]["init_args"]["end_filter"]["init_args"]


def _draw(rng, *shape_m1):
    """mc[0] in U(-3, 3), mc[m] = N(0, 1) 0.8^m: |Re L| stays near 20 at the most, well inside the range of fp32 exp"""
    mc = rng.normal(0, 1, shape_m1) * 0.8 ** np.arange(shape_m1[-1])
    mc[..., 0] = rng.uniform(-3, 3, shape_m1[:-1])
    return mc


def test_class_resolves_and_the_diffsptk_classes_do_not():
    from golf_amd.config import resolve_class
    from golf_amd.filters import LTVMLSAFilter2

    assert resolve_class("models.filters.LTVMLSAFilter2") is LTVMLSAFilter2
    for name in ("LTVMLSAFilter", "LTVAPFilter"):
        with pytest.raises(NotImplementedError, match="no counterpart"):
            resolve_class("models.filters." + name)


def test_converted_config_builds_the_mlsa_decoder():
    from golf_amd.ae import VoiceAutoEncoder
    from golf_amd.config import build_model, mlsa_to_stft_filter
    from golf_amd.filters import LTVMLSAFilter2

    cfg = _config()
    with pytest.raises(NotImplementedError, match="LTVMLSAFilter"):
        build_model(cfg)                       # diffsptk's own framing stays unresolved: the rewrite is an opt-in
    before = copy.deepcopy(cfg)
    out = mlsa_to_stft_filter(cfg)
    assert cfg == before                       # a deep copy: the input is untouched
    node = out["model"]["init_args"]["decoder"]["init_args"]["end_filter"]
    assert node == {"class_path": "models.filters.LTVMLSAFilter2",
                    "init_args": {"n_fft": 1024, "frame_period": 240, "filter_order": 24, "alpha": 0.46, "gamma": 0,
                                  "window": "hanning"}}
    model = build_model(out)
    assert isinstance(model, VoiceAutoEncoder)
    f = model.decoder.end_filter
    assert type(f) is LTVMLSAFilter2 and f.hip_frames is True
    assert (f.n_fft, f.hop_length, f.filter_order, f.alpha) == (1024, 240, 24, 0.46)
    assert f._window.shape == (1024,) and f._window.dtype == torch.float32
    assert f.ctrl.split_size == (25,)
    sizes, _, keys = model.decoder.split_sizes_and_trsfms
    assert sizes[keys.index("end_filter_params")] == (25,)
    x = torch.randn(2, 3, 25)
    assert f.ctrl.trsfm_fn(x)[0] is x          # the mel cepstrum is the encoder head's output as it is
    assert "_basis" not in f.state_dict() and "_window" not in f.state_dict()


@pytest.mark.parametrize("field,value", [("mode", "multi-stage"), ("phase", "zero"), ("gamma", -0.5), ("c", 2),
                                         ("ignore_gain", True), ("frame_length", 512)])
def test_config_rewrite_refuses(field, value):
    from golf_amd.config import mlsa_to_stft_filter

    cfg = _config()
    _end_filter_args(cfg)[field] = value
    with pytest.raises(NotImplementedError, match=field):
        mlsa_to_stft_filter(cfg)


def test_constructor_refusals():
    from golf_amd.filters import LTVMLSAFilter2

    with pytest.raises(NotImplementedError, match="gamma"):
        LTVMLSAFilter2(1024, 240, 24, gamma=-0.5)
    with pytest.raises(NotImplementedError, match="positional"):
        LTVMLSAFilter2(1024, 240, 24, 7)
    with pytest.raises(NotImplementedError, match="taylor_order"):
        LTVMLSAFilter2(1024, 240, 24, taylor_order=20)
    with pytest.raises(NotImplementedError, match="phase"):
        LTVMLSAFilter2(1024, 240, 24, phase="zero")
    f = LTVMLSAFilter2(1024, 240, 24, alpha=0.46, c=None, ignore_gain=False, phase="minimum", mode="freq-domain",
                       frame_length=1024, fft_length=1024)       # the MLSA defaults a saved config spells out
    assert f.n_fft == 1024


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_module_path_matches_the_references_own_run(golden, tag):
    """y and both gradients within 1e-10 of max|y|: this definition and the reference's truncate-and-Hilbert formulation agree
    to 5e-15 in log H at n_fft >= 256, and the framing is the same torch.stft / torch.istft pair."""
    from golf_amd.audiotensor import AudioTensor as AT
    from golf_amd.filters import LTVMLSAFilter2

    g = golden("g31_mlsa_filter")
    n, hop, M, alpha = (int(g[f"{tag}_n_fft"]), int(g[f"{tag}_hop"]), int(g[f"{tag}_order"]), float(g[f"{tag}_alpha"]))
    f = LTVMLSAFilter2(n, hop, M, window="hanning", alpha=alpha).double()
    ex = torch.tensor(g[f"{tag}_ex"], requires_grad=True)
    mc = torch.tensor(g[f"{tag}_mc"], requires_grad=True)
    y = f(AT(ex), AT(mc, hop)).as_tensor()
    assert y.dtype == torch.float64 and y.shape == g[f"{tag}_y"].shape
    assert y.shape[1] == hop * (min(1 + ex.shape[1] // hop, mc.shape[1]) - 1)
    g_ex, g_mc = torch.autograd.grad((y * torch.tensor(g[f"{tag}_gy"])).sum(), (ex, mc))
    scale = np.abs(g[f"{tag}_y"]).max()
    errs = [np.abs(got.detach().numpy() - g[f"{tag}_{k}"]).max() / scale for got, k in ((y, "y"), (g_ex, "g_ex"), (g_mc, "g_mc"))]
    print(f"g31{tag}: y, g_ex, g_mc vs the reference's run, relative to max|y|:", errs)
    assert max(errs) <= 1e-10, errs
    if mc.shape[1] > 1 + ex.shape[1] // hop:          # the control row no frame uses
        assert np.all(g_mc.numpy()[:, 1 + ex.shape[1] // hop:] == 0)


@pytest.mark.parametrize("n,M,alpha", [(64, 24, 0.46), (256, 64, -0.3), (1024, 24, 0.46), (2048, 64, 0.77), (1000, 5, 0.1)])
def test_numpy_definition_matches_the_torch_composition(n, M, alpha):
    from golf_amd import functional as GF

    rng = np.random.default_rng(n + M)
    mc = _draw(rng, 3, 4, M + 1)
    want = mlsa_ref.response(mc, n, alpha)
    t = torch.tensor(mc, requires_grad=True)
    got = GF.mel_cepstrum_response(t, n, alpha)
    assert got.dtype == torch.complex128 and got.shape == (3, 4, n // 2 + 1)
    assert np.abs(got.detach().numpy() - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(got.detach().numpy().imag[..., [0, -1]] == 0)
    g_h = rng.normal(0, 1, want.shape) + 1j * rng.normal(0, 1, want.shape)
    (g_mc,) = torch.autograd.grad(torch.view_as_real(got), t, torch.view_as_real(torch.tensor(g_h)), retain_graph=True)
    want_g = mlsa_ref.response_bwd(g_h, mc, n, alpha)
    assert np.abs(g_mc.numpy() - want_g).max() <= 1e-12 * np.abs(want_g).max()
    # torch's convention for a complex cotangent is the one the kernel's backward takes
    (g_mc2,) = torch.autograd.grad(got, t, torch.tensor(g_h))
    assert np.abs(g_mc2.numpy() - want_g).max() <= 1e-12 * np.abs(want_g).max()


def test_alpha_zero_is_the_cepstral_filter():
    """alpha = 0: theta_k = w_k, so the rows are LTVCepFilter(phase="min")'s on ceps = (mc_0, mc_1 / 2, ...): its log
    magnitude is c_0 + 2 sum_m c_m cos(m w_k) and its Hilbert phase that of the same causal cepstrum."""
    from golf_amd.filters import LTVCepFilter, LTVMLSAFilter2

    n, M = 256, 24
    mc = torch.tensor(_draw(np.random.default_rng(7), 2, 5, M + 1))
    ceps = mc.clone()
    ceps[..., 1:] /= 2
    a = LTVMLSAFilter2(n, 64, M, alpha=0).response_rows(mc)
    b = LTVCepFilter(M, n, "hanning", 64, phase="min").response_rows(ceps)
    assert a.shape == b.shape == (2, 5, n // 2 + 1)
    assert (a - b).abs().max() <= 1e-12 * b.abs().max()
    full = LTVMLSAFilter2(n, 64, M, alpha=0).frequency_response(mc)
    want = LTVCepFilter(M, n, "hanning", 64, phase="min").frequency_response(ceps)
    assert full.shape == want.shape == (2, n, 5) and (full - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize("n,M,alpha", [(1024, 24, 0.46), (2048, 64, 0.77)])
def test_fit_recovers_the_mel_cepstrum(n, M, alpha):
    from golf_amd.filters import LTVMLSAFilter2

    mc = _draw(np.random.default_rng(M), 2, 3, M + 1)
    log_env = torch.tensor(mlsa_ref.log_response(mc, n, alpha).real)
    f = LTVMLSAFilter2(n, n // 4, M, alpha=alpha)
    got = f.fit(log_env)
    assert got.shape == (2, 3, M + 1) and got.dtype == torch.float64
    assert np.abs(got.numpy() - mc).max() <= 1e-9
    assert f.fit(log_env.float()).dtype == torch.float32
    with pytest.raises(ValueError):
        f.fit(log_env[..., :-1])


def test_stream_branch_kind_and_cpu_fallbacks():
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError
    from golf_amd.filters import LTVMLSAFilter2
    from golf_amd.stream import _branch_kind

    assert _branch_kind(LTVMLSAFilter2(64, 16, 8, alpha=0.3)) == "stft"

    class Sub(LTVMLSAFilter2):
        pass

    assert _branch_kind(Sub(64, 16, 8)) is None
    assert GF.mel_cepstrum_kernel_takes(1024, 24, 0.46) and GF.mel_cepstrum_kernel_takes(64, 0, -0.99)
    assert not GF.mel_cepstrum_kernel_takes(1000, 24, 0.46) and not GF.mel_cepstrum_kernel_takes(1024, 65, 0.46)
    assert not GF.mel_cepstrum_kernel_takes(32, 4, 0.0) and not GF.mel_cepstrum_kernel_takes(4096, 4, 0.0)
    assert not GF.mel_cepstrum_kernel_takes(1024, 24, 1.0)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.mel_cepstrum_rows(torch.zeros(2, 25), torch.zeros(8), 1024)
    with pytest.raises(GolfError, match="no CPU path"):
        GF.mel_cepstrum_basis(1024, 24, 0.46, "cpu")


def test_argument_checks_without_gpu():
    """Bad arguments are refused before any launch, so these calls are safe on a GPU-less host; the pointers that are not
    null are never dereferenced."""
    from golf_amd import _lib

    lib = _lib.load()
    K = lambda n: n // 2 + 64
    assert lib.golf_mlsa_response_basis_bytes(1024, 24) == 2 * 25 * K(1024) * 4
    assert lib.golf_mlsa_response_basis_bytes(64, 0) == 2 * 1 * K(64) * 4
    assert lib.golf_mlsa_response_basis_bytes(2048, 64) == 2 * 65 * K(2048) * 4
    for n, m in ((1000, 24), (32, 24), (4096, 24), (1024, 65), (1024, -1)):
        assert lib.golf_mlsa_response_basis_bytes(n, m) == 0
    big, p = 1 << 20, 4096   # a pointer that is not null
    err = lambda: lib.golf_last_error()
    assert lib.golf_mlsa_response_basis_f32(1024, 24, 0.46, None, big, None) == -1 and b"null" in err()
    assert lib.golf_mlsa_response_basis_f32(1000, 24, 0.46, p, big, None) == -3 and b"power of two" in err()
    assert lib.golf_mlsa_response_basis_f32(32, 24, 0.46, p, big, None) == -3
    assert lib.golf_mlsa_response_basis_f32(1024, 65, 0.46, p, big, None) == -3 and b"order" in err()
    assert lib.golf_mlsa_response_basis_f32(1024, -1, 0.46, p, big, None) == -3
    for alpha in (1.0, -1.0, 1.5, float("nan")):
        assert lib.golf_mlsa_response_basis_f32(1024, 24, alpha, p, big, None) == -1 and b"alpha" in err()
    need = lib.golf_mlsa_response_basis_bytes(1024, 24)
    assert lib.golf_mlsa_response_basis_f32(1024, 24, 0.46, p, need - 4, None) == -2 and b"bytes" in err()
    for fn, nulls in ((lib.golf_mlsa_response_rows_f32, ((None, p, p), (p, None, p), (p, p, None))),):
        for mc, basis, h in nulls:
            assert fn(mc, basis, big, h, 4, 1024, 24, None) == -1 and b"null" in err()
    assert lib.golf_mlsa_response_rows_f32(p, p, big, p, 4, 1000, 24, None) == -3
    assert lib.golf_mlsa_response_rows_f32(p, p, big, p, 4, 1024, 65, None) == -3
    assert lib.golf_mlsa_response_rows_f32(p, p, need - 4, p, 4, 1024, 24, None) == -2
    assert lib.golf_mlsa_response_rows_f32(p, p, big, p, -1, 1024, 24, None) == -1
    assert lib.golf_mlsa_response_rows_f32(p, p, big, p, 0, 1024, 24, None) == 0          # R = 0 does nothing
    for g_h, mc, basis, g_mc in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.golf_mlsa_response_rows_bwd_f32(g_h, mc, basis, big, g_mc, 4, 1024, 24, None) == -1 and b"null" in err()
    assert lib.golf_mlsa_response_rows_bwd_f32(p, p, p, big, p, 4, 1000, 24, None) == -3
    assert lib.golf_mlsa_response_rows_bwd_f32(p, p, p, big, p, 4, 2048, 65, None) == -3
    assert lib.golf_mlsa_response_rows_bwd_f32(p, p, p, need - 4, p, 4, 1024, 24, None) == -2
    assert lib.golf_mlsa_response_rows_bwd_f32(p, p, p, big, p, -2, 1024, 24, None) == -1
    assert lib.golf_mlsa_response_rows_bwd_f32(p, p, p, big, p, 0, 1024, 24, None) == 0
