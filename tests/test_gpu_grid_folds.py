"""The 2-D grid fold of the six launches with one workgroup per frame or tile: f0_yin_kernel and f0_candidates_kernel
(YIN_GRID_X), harm_analysis_kernel (HNA_GRID_X), spec_envelope_kernel (ENV_GRID_X), the glottal match (GM_GRID_X) and
ltv_residual_kernel (RES_GRID_X).  Each launches dim3(min(G, 2^20), ceil(G / 2^20)) workgroups, recovers
g = blockIdx.y * gridDim.x + blockIdx.x and leaves the ragged last grid row by ``g >= G``; below 2^20 frames blockIdx.y is
always 0, so every test here launches G just above 2^20.

A float64 reference of a million frames is not needed: the kernels are batch independent (each parity file asserts it), so
the big batch is made of tiled copies of a small case of ``nb`` rows and row b of the big result must have the bits of row
b % nb of the small one.  The small cases are held to float64 by the parity files (f0_ref small50, hna_ref hop1, env_ref n64,
glottal_ref smallest, and the one-tile case of tests/test_gpu_residual.py); here the small result through the C entry is
tied to the Python wrapper's, bit for bit.

Every call goes through the C entries with outputs pre-filled with a NaN of a payload that no kernel produces: a frame that
no workgroup wrote keeps it and fails the comparison, whatever the frame's own value is (the match writes NaN itself)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FOLD = 1 << 20          # workgroups per grid row: *_GRID_X of the six launches
FILL = 0x7FC0DEAD       # a quiet NaN with a payload: not the NaN of 0/0 or of a kernel's ``no estimate``


def filled(*shape):
    return torch.full(shape, FILL, dtype=torch.int32, device="cuda").view(torch.float32)


def bits(t):
    assert t.dtype == torch.float32 and t.is_contiguous()
    return t.view(torch.int32)


def tiled(small, B):
    """(nb, ...) -> (B, ...): row b is row b % nb."""
    small = small if isinstance(small, torch.Tensor) else torch.tensor(small).cuda()
    reps = -(-B // small.shape[0])
    return small.repeat((reps,) + (1,) * (small.dim() - 1))[:B].contiguous()


def crosses_the_fold(G):
    assert G > FOLD          # blockIdx.y reaches 1
    assert G % FOLD != 0     # and the last grid row is partial: ``g >= G`` ends workgroups


def rows_repeat(what, big, small, wrapper=None):
    """Every value of ``big`` (B, ...) and ``small`` (nb, ...) was written, row b of big has the bits of row b % nb of small,
    and small has the bits of the Python wrapper's result."""
    bb, sb = bits(big), bits(small)
    nb, B = small.shape[0], big.shape[0]
    reps, tail = divmod(B, nb)
    assert reps > 1 and big.shape[1:] == small.shape[1:]
    assert not (sb == FILL).any(), what
    assert not (bb == FILL).any(), (what, int((bb == FILL).sum()))
    if wrapper is not None:
        assert torch.equal(sb, bits(wrapper.contiguous())), what
    assert (bb[:reps * nb].view(reps, *sb.shape) == sb).all(), what
    assert torch.equal(bb[reps * nb:], sb[:tail]), what


def yin_case():
    import f0_ref as R
    from test_gpu_f0 import run

    x, kw = R.cases()["small50"]
    F = R.reference("small50")["f0"].shape[1]
    B = -(-(FOLD + 1) // F)   # the smallest batch that crosses the fold
    assert (x.shape[0], F, B) == (5, 112, 9363)
    return x, kw, F, B, run


def test_f0_yin():
    from golf_amd import _lib

    lib = _lib.load()
    x, kw, F, B, run = yin_case()
    crosses_the_fold(B * F)
    S = kw["W"] + kw["tau_max"]

    def call(xd):
        out = filled(3, xd.shape[0], F)
        rc = lib.golf_f0_yin_f32(xd.data_ptr(), xd.stride(0), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                 xd.shape[0], xd.shape[1], F, kw["hop"], kw["W"], kw["tau_min"], kw["tau_max"], -(S // 2),
                                 kw["sample_rate"], kw["threshold"], 0.0, _lib.stream_ptr())
        _lib.check(rc, "golf_f0_yin_f32")
        return out

    small, big = call(tiled(x, x.shape[0])), call(tiled(x, B))
    assert (small[0] > 0).any() and (small[0] == 0).any()   # voiced and unvoiced frames
    for i, (name, own) in enumerate(zip(("f0", "period", "ap"), run(x, kw))):
        rows_repeat(name, big[i], small[i], own)


def test_f0_candidates():
    from golf_amd import _lib
    from test_gpu_f0_track import run_cand

    lib = _lib.load()
    x, kw, F, B, _ = yin_case()
    crosses_the_fold(B * F)
    K, S = 3, kw["W"] + kw["tau_max"]

    def call(xd):
        out = filled(2, xd.shape[0], F, K)
        rc = lib.golf_f0_candidates_f32(xd.data_ptr(), xd.stride(0), out[0].data_ptr(), out[1].data_ptr(), xd.shape[0],
                                        xd.shape[1], F, kw["hop"], kw["W"], kw["tau_min"], kw["tau_max"], K, -(S // 2), 0.0,
                                        _lib.stream_ptr())
        _lib.check(rc, "golf_f0_candidates_f32")
        return out

    small, big = call(tiled(x, x.shape[0])), call(tiled(x, B))
    assert (small[0] > 0).any()
    for i, (name, own) in enumerate(zip(("period", "ap"), run_cand(x, kw, K))):
        rows_repeat(name, big[i], small[i], own)


def test_harmonic_analysis():
    import hna_ref as R
    from golf_amd import _lib
    from test_gpu_hna import run

    lib = _lib.load()
    x, f0, kw = R.cases()["hop1"]
    assert kw == dict(sample_rate=kw["sample_rate"], hop=1, K=12, n_mag=33)   # the defaults below are the wrapper's
    (nb, T), F, K, n_mag, hop = x.shape, f0.shape[1], kw["K"], kw["n_mag"], kw["hop"]
    B = 16133
    assert (nb, T, F) == (1, 64, 65)
    crosses_the_fold(B * F)

    def call(xd, fd):
        n = xd.shape[0]
        out = [filled(n, F, w) for w in (K, K, n_mag)]
        rc = lib.golf_harmonic_analysis_f32(xd.data_ptr(), xd.stride(0), fd.data_ptr(), fd.stride(0), out[0].data_ptr(),
                                            out[1].data_ptr(), out[2].data_ptr(), n, T, F, K, n_mag, hop, 4, 2 * hop, 2048,
                                            4 * hop, 0, kw["sample_rate"], 1e-12, _lib.stream_ptr())
        _lib.check(rc, "golf_harmonic_analysis_f32")
        return out

    small, big = call(tiled(x, nb), tiled(f0, nb)), call(tiled(x, B), tiled(f0, B))
    assert (small[0] > 0).any()
    for name, b, s, own in zip(("amp", "phases", "log_mag"), big, small, run(x, f0, kw)):
        rows_repeat(name, b, s, own)


def test_spectral_envelope():
    import env_ref as R
    from golf_amd import _lib
    from test_gpu_env import run

    lib = _lib.load()
    x, f0, kw = R.cases()["n64"]
    (nb, T), F, n, hop, sr = x.shape, f0.shape[1], kw["n_fft"], kw["hop"], kw["sample_rate"]
    B = -(-(FOLD + 1) // F)
    assert (nb, T, F, n, B) == (3, 65, 9, 64, 116509)
    crosses_the_fold(B * F)
    lo, hi = R.defaults(sr, n)

    def call(xd, fd):
        m = xd.shape[0]
        out = [filled(m, F, n // 2 + 1), filled(m, F, n // 2 + 1)]
        rc = lib.golf_spectral_envelope_f32(xd.data_ptr(), xd.stride(0), fd.data_ptr(), fd.stride(0), out[0].data_ptr(),
                                            out[1].data_ptr(), m, T, F, n, n // 2 + 1, hop, sr, lo, hi, kw["unvoiced_f0"],
                                            -0.15, 1e-12, R.OFFSET, _lib.stream_ptr())
        _lib.check(rc, "golf_spectral_envelope_f32")
        return out

    small, big = call(tiled(x, nb), tiled(f0, nb)), call(tiled(x, B), tiled(f0, B))
    for name, b, s, own in zip(("log_env", "ceps"), big, small, run(x, f0, kw)):
        rows_repeat(name, b, s, own)


def test_glottal_match():
    import glottal_ref as R
    from golf_amd import _lib
    from test_gpu_glottal import plan_of, run

    lib = _lib.load()
    c = R.cases()["smallest"]
    own, (amp, ph) = run("smallest")   # the match of the parity test, on the harmonics the kernel in front of it gives
    nb, F, H = amp.shape
    f0 = torch.tensor(c["f0"]).cuda()
    B = -(-(FOLD + 1) // F)
    assert (nb, F, H, B) == (1, 9, 1, 116509)
    crosses_the_fold(B * F)
    plan = plan_of("smallest")
    S, N, X = plan.spectrum, plan.norms, plan.cross

    def call(ad, pd, fd):
        m = ad.shape[0]
        out = filled(3, m, F)
        rc = lib.golf_glottal_match_f32(ad.data_ptr(), pd.data_ptr(), fd.data_ptr(), fd.stride(0), S.data_ptr(), N.data_ptr(),
                                        X.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), m, F, H,
                                        S.shape[0], c["n_phi"], c["sample_rate"], _lib.stream_ptr())
        _lib.check(rc, "golf_glottal_match_f32")
        return out

    small, big = call(tiled(amp, nb), tiled(ph, nb), tiled(f0, nb)), call(tiled(amp, B), tiled(ph, B), tiled(f0, B))
    assert torch.isfinite(small[0]).any()   # frames with an estimate
    for i, name in enumerate(("w", "theta", "rho")):
        rows_repeat(name, big[i], small[i], own[i])


def test_ltv_residual():
    import residual_ref as R
    from golf_amd import _lib
    from golf_amd import functional as GF
    from test_gpu_residual import CASES, inputs

    lib = _lib.load()
    case = nb, F, M, hop, T = 8, 2, 2, 7, 8   # one tile per row: G = B
    assert case in CASES                      # held to float64 there
    x, gain, a = inputs(case)
    B = FOLD + 24
    n_out = R.length(T, F, hop)
    assert n_out == T <= 256 and B % nb == 0
    crosses_the_fold(B)

    def call(xd, gd, ad):
        m = xd.shape[0]
        e = filled(m, n_out)
        rc = lib.golf_ltv_residual_f32(xd.data_ptr(), xd.stride(0), gd.data_ptr(), ad.data_ptr(), e.data_ptr(), e.stride(0), m,
                                       T, F, M, hop, _lib.stream_ptr())
        _lib.check(rc, "golf_ltv_residual_f32")
        return e

    small = call(tiled(x, nb), tiled(gain, nb), tiled(a, nb))
    big = call(tiled(x, B), tiled(gain, B), tiled(a, B))
    own = GF.ltv_residual(torch.tensor(x).cuda(), torch.tensor(gain).cuda(), torch.tensor(a).cuda(), hop)
    assert np.isfinite(small.cpu().numpy()).all()
    rows_repeat("e", big, small, own)
