"""CPU: the host side of the minimum-phase FIR filters -- C entries declared, bound and exported, argument checks
without a GPU, config rewriting and class resolution, and the float64 restatement (tests/minphase_ref.py) against the
reference's own output (tests/golden/g29, g30)."""
import copy
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import minphase_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["golf_min_phase_fir_basis_bytes", "golf_min_phase_fir_basis_f32", "golf_min_phase_fir_kernels_f32",
       "golf_min_phase_fir_kernels_bwd_f32", "golf_ltv_fir_frames_causal_length", "golf_ltv_fir_frames_causal_fwd_f32",
       "golf_ltv_fir_frames_causal_bwd_f32"]


def prototype(name):
    text = open(os.path.join(ROOT, "include", "golf_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared in include/golf_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_exports_and_binding_agree():
    import ctypes

    from golf_amd import _lib

    _lib.build()
    lib = _lib.load()
    assert lib.golf_abi_version() == _lib.ABI_VERSION == 6   # additive: the ABI version stays
    assert "minphase_fir.hip" in _lib.SOURCES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (golf_[a-z0-9_]+)", out))
    kinds = {ctypes.c_int: "int", ctypes.c_int64: "int64_t", ctypes.c_size_t: "size_t", ctypes.c_void_p: "*"}
    for name in NEW:
        assert name in exported and name in _lib.SIGNATURES
        args = prototype(name)
        _, argtypes = _lib.SIGNATURES[name]
        assert len(args) == len(argtypes), (name, args)
        for decl, ct in zip(args, argtypes):   # pointers bind as void*, scalars by their C type
            want = kinds[ct]
            assert ("*" in decl) == (want == "*") and (want == "*" or decl.split()[-2] == want), (name, decl, want)
    text = open(os.path.join(ROOT, "include", "golf_amd.h")).read()
    assert "models/filters.py:203-221" in text and "models/filters.py:270-283" in text   # the lines the entries replace


def test_argument_checks_without_gpu():
    """Bad arguments are refused before any launch, so these calls are safe on a host without a GPU."""
    from golf_amd import _lib

    lib = _lib.load()
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -2
    assert lib.golf_min_phase_fir_basis_bytes(1) == 0
    # S both ways (256^2 each) + [C; -Sn] both ways (512 x 512 each), floats
    assert lib.golf_min_phase_fir_basis_bytes(256) == (2 * 256 * 256 + 2 * 512 * 512) * 4
    assert lib.golf_min_phase_fir_basis_bytes(9) == (2 * 128 * 128 + 2 * 256 * 128) * 4
    assert lib.golf_min_phase_fir_basis_f32(1, None, 0, None) == EINVAL
    assert lib.golf_min_phase_fir_basis_f32(9, None, 1 << 20, None) == EINVAL and b"min_phase_fir_basis" in lib.golf_last_error()
    fake = 256   # never dereferenced: every call below is refused before a launch
    assert lib.golf_min_phase_fir_basis_f32(9, fake, 16, None) == EWORKSPACE
    assert lib.golf_min_phase_fir_kernels_f32(None, None, None, None, 4, 9, None) == EINVAL
    assert b"min_phase_fir_kernels" in lib.golf_last_error()
    assert lib.golf_min_phase_fir_kernels_f32(fake, fake, fake, fake, 0, 9, None) == EINVAL
    assert lib.golf_min_phase_fir_kernels_f32(fake, fake, fake, fake, 4, 1, None) == EINVAL
    assert lib.golf_min_phase_fir_kernels_bwd_f32(None, None, None, None, None, 4, 9, None) == EINVAL
    assert lib.golf_min_phase_fir_kernels_bwd_f32(fake, fake, fake, fake, fake, 4, 1, None) == EINVAL
    # rows that do not fit the LDS of one workgroup are refused, not truncated
    assert lib.golf_min_phase_fir_kernels_f32(fake, fake, fake, fake, 4, 2000, None) == EUNSUPPORTED
    assert lib.golf_min_phase_fir_kernels_bwd_f32(fake, fake, fake, fake, fake, 4, 2000, None) == EUNSUPPORTED
    # causal frame FIR: T // hop frames, capped at F; -1 where there is not one hop of signal
    assert lib.golf_ltv_fir_frames_causal_length(1000, 9, 64, 240) == 960
    assert lib.golf_ltv_fir_frames_causal_length(1000, 3, 64, 240) == 720
    assert lib.golf_ltv_fir_frames_causal_length(240, 3, 510, 240) == 240   # the zero-phase one needs T >= hop + (N-1) - 2P
    assert lib.golf_ltv_fir_frames_causal_length(239, 3, 64, 240) == -1
    assert lib.golf_ltv_fir_frames_causal_fwd_f32(None, 0, None, 64, None, 0, 2, 1000, 4, 64, 240, 0, None) == EINVAL
    assert b"ltv_fir_frames_causal_fwd" in lib.golf_last_error()
    assert lib.golf_ltv_fir_frames_causal_fwd_f32(fake, 0, fake, 60, fake, 0, 2, 1000, 4, 64, 240, 0, None) == EINVAL   # row stride < N
    assert lib.golf_ltv_fir_frames_causal_fwd_f32(fake, 0, fake, 64, fake, 0, 2, 1000, 4, 64, 240, 4, None) == EINVAL   # frame0 >= F
    assert lib.golf_ltv_fir_frames_causal_bwd_f32(None, 0, None, 0, None, 64, None, 0, None, 2, 1000, 4, 64, 240, 0, None) == EINVAL
    assert lib.golf_ltv_fir_frames_causal_bwd_f32(fake, 0, fake, 0, fake, 64, fake, 0, fake, 2, 1000, 4, 64, 243, 0, None) == EUNSUPPORTED
    assert b"ltv_fir_frames_causal_bwd: hop=243 must be a multiple of 4" in lib.golf_last_error()
    # the twin's entries answer as before
    assert lib.golf_ltv_fir_frames_length(1000, 9, 64, 240) == 960 and lib.golf_ltv_fir_frames_length(240, 3, 510, 240) == -1
    assert lib.golf_ltv_fir_frames_bwd_f32(fake, 0, fake, 0, fake, 64, fake, 0, fake, 2, 1000, 4, 64, 243, 0, None) == EUNSUPPORTED
    assert b"ltv_fir_frames_bwd: hop=243 must be a multiple of 4" in lib.golf_last_error()


def test_convert2samplewise_rewrites_the_new_class():
    from golf_amd.filters import convert2samplewise

    cfg = {"decoder": {"class_path": "models.sf.SourceFilterSynth", "init_args": {
        "noise_filter": {"class_path": "models.filters.LTVMinimumPhaseFIRFilter",
                         "init_args": {"window": "hanning", "conv_method": "direct", "n_mag": 256}},
        "end_filter": {"class_path": "models.filters.LTVMinimumPhaseFilter",
                       "init_args": {"window": "hanning", "window_length": 960, "centred": True, "lpc_order": 22}},
        "other": {"class_path": "models.filters.LTVZeroPhaseFIRFilter",
                  "init_args": {"window": "hanning", "conv_method": "fft", "n_mag": 256}}}}}
    out = convert2samplewise(copy.deepcopy(cfg))["decoder"]["init_args"]
    assert out["noise_filter"] == {"class_path": "models.filters.LTVMinimumPhaseFIRFilterPrecise",
                                   "init_args": {"window": "hanning", "n_mag": 256}}
    # the two branches that were there give what they gave
    assert out["end_filter"] == {"class_path": "models.filters.LTVMinimumPhaseFilterPrecise", "init_args": {"lpc_order": 22}}
    assert out["other"] == {"class_path": "models.filters.LTVZeroPhaseFIRFilterPrecise",
                            "init_args": {"window": "hanning", "n_mag": 256}}
    # already sample-wise: untouched; this package's own module path works too
    done = {"class_path": "golf_amd.filters.LTVMinimumPhaseFIRFilterPrecise", "init_args": {"window": "hanning"}}
    assert convert2samplewise(copy.deepcopy(done)) == done
    own = convert2samplewise({"class_path": "golf_amd.filters.LTVMinimumPhaseFIRFilter",
                              "init_args": {"window": "hamming", "conv_method": "fft"}})
    assert own == {"class_path": "golf_amd.filters.LTVMinimumPhaseFIRFilterPrecise", "init_args": {"window": "hamming"}}


def test_build_model_resolves_the_new_classes():
    from golf_amd import filters
    from golf_amd.config import build_model, resolve_class

    for name in ("LTVMinimumPhaseFIRFilterPrecise", "LTVMinimumPhaseFIRFilter", "LTIRadiationFilter",
                 "SampleBasedLTVMinimumPhaseFilter"):
        assert resolve_class(f"models.filters.{name}") is getattr(filters, name)
    fw = build_model({"decoder": {"class_path": "models.filters.LTVMinimumPhaseFIRFilter",
                                  "init_args": {"window": "hanning", "conv_method": "fft", "n_mag": 256}}})
    assert type(fw) is filters.LTVMinimumPhaseFIRFilter and fw.ctrl.split_size == (256,)
    pr = build_model({"decoder": {"class_path": "models.filters.LTVMinimumPhaseFIRFilterPrecise",
                                  "init_args": {"window": "hamming"}}})
    assert type(pr) is filters.LTVMinimumPhaseFIRFilterPrecise and pr.ctrl.split_size == ()
    assert isinstance(fw, filters.LTVMinimumPhaseFIRFilterPrecise)
    with pytest.raises(ValueError, match="conv_method"):
        filters.LTVMinimumPhaseFIRFilter(window="hanning", conv_method="overlap-save")
    w = pr.windowing(torch.ones(2, 16))   # the tail half of the window only
    assert torch.equal(w[:, :8], torch.ones(2, 8)) and torch.allclose(w[0, 8:], torch.hamming_window(16)[8:])
    rad = build_model({"decoder": {"class_path": "models.filters.LTIRadiationFilter", "init_args": {"num_zeros": 16}}})
    assert rad._kernel.shape == (1, 1, 33) and rad._padding == 16 and not rad.state_dict()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        old = build_model({"decoder": {"class_path": "models.filters.SampleBasedLTVMinimumPhaseFilter",
                                       "init_args": {"lpc_order": 22}}})
    assert any("deprecated" in str(w.message) for w in seen)
    assert isinstance(old, filters.LTVMinimumPhaseFilterPrecise) and old.ctrl.split_size == (1, 22)
    # what still has no drop-in stays refused
    for name in ("LTIComplexConjAllpassFilter", "LTIRealCoeffAllpassFilter", "LTVPQMF", "LTVMLSAFilter", "LTVAPFilter"):
        with pytest.raises(NotImplementedError):
            resolve_class(f"models.filters.{name}")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_reproduces_g29(golden, tag):
    g = golden("g29_min_phase_fir")
    ex, lm, hop, window = g[f"{tag}_ex"], g[f"{tag}_log_mag"], int(g[f"{tag}_hop"]), str(g[f"{tag}_window"])
    assert str(g[f"{tag}_frame_path"]) in ("forward", "steps") and str(g[f"{tag}_precise_path"]) in ("forward", "steps")
    n_mag = lm.shape[-1]
    N = 2 * (n_mag - 1)
    win = R.min_phase_window(window, N)
    k = R.min_phase_kernels(torch.tensor(lm), win).numpy()
    assert np.abs(k - g[f"{tag}_kernel"]).max() <= 1e-12
    Ccep, Sth, _, _ = R.design_matrices(n_mag)
    theta = ((torch.tensor(lm[:, 0]) @ Ccep.T) @ Sth.T).numpy()
    assert np.abs(theta - g[f"{tag}_theta"]).max() <= 1e-12 and np.abs(theta[:, [0, -1]]).max() <= 1e-14
    for pre, sw in (("", False), ("p_", True)):
        y, gx, glm = R.filter_with_grads(ex, lm, win, hop, g[f"{tag}_{pre}gy"], samplewise=sw)
        assert y.shape == g[f"{tag}_{pre}y"].shape
        assert np.abs(y - g[f"{tag}_{pre}y"]).max() <= 1e-12
        assert np.abs(gx - g[f"{tag}_{pre}g_ex"]).max() <= 1e-12
        assert np.abs(glm - g[f"{tag}_{pre}g_log_mag"]).max() <= 1e-12


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_radiation_time_filter_reproduces_g30(golden, tag):
    from golf_amd.utils import get_radiation_time_filter, get_window_fn

    g = golden("g30_radiation_filter")
    nz, window = int(g[f"{tag}_num_zeros"]), str(g[f"{tag}_window"])
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        taps = get_radiation_time_filter(nz, get_window_fn(window))
        plain = get_radiation_time_filter(nz)
    finally:
        torch.set_default_dtype(before)
    assert taps.dtype == torch.float64 and taps.shape == (2 * nz + 1,)
    assert np.abs(taps.numpy() - g[f"{tag}_taps"]).max() <= 1e-12
    assert np.abs(plain.numpy() - g[f"{tag}_taps_plain"]).max() <= 1e-12
    assert np.abs(taps.flip(0).numpy() - g[f"{tag}_module_kernel"][0, 0]).max() <= 1e-12
    # same-length correlation with the flipped taps is what the module's forward computes
    ex, k = g[f"{tag}_ex"], g[f"{tag}_module_kernel"][0, 0]
    y = np.stack([np.correlate(np.pad(r, nz), k, mode="valid") for r in ex])
    assert np.abs(y - g[f"{tag}_y"]).max() <= 1e-12
