"""GPU tests of the packed-FIR family of csrc/noise_fir.hip on its own -- lti_fir_kernel<REV>, lti_fir_taps_grad_kernel
(+ reduce), fir_frames_{fwd,bwd_kern,bwd_ex}_kernel<CAUSAL> -- and of the oscillator's decimator and its two transposes
(csrc/glottal_osc.hip: osc_decimate_kernel<OST>, osc_decimate_T_kernel, osc_decimate_T4_kernel), at every tile edge, with
random ASYMMETRIC taps, against the plain float64 references of tests/fir_ref.py.  tests/test_fir_ref_host.py shows on the
CPU that these very inputs tell a mirrored row, an off-by-one lead or offset, a dropped tap, a wrong kernel row, an omitted
ragged tail and a stale unused row from the right answer by >= 100 bars, and that a sequential float32 sum stays within a
third of them.  Bars: 1e-5 forward, 2e-5 gradients, both norms of conftest.rel_err."""
import functools

import numpy as np
import pytest
import torch

import fir_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
WORST = {}          # group -> worst rel-max seen so far


def dev(x, grad=False):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda().requires_grad_(grad)


def host(t):
    return t.detach().cpu().numpy()


def check(got, ref, what, bar, group):
    got = np.asarray(got)
    emax, el2 = rel_err(got, ref)
    WORST[group] = max(WORST.get(group, 0.0), emax)
    print(f"{what}: rel-max {emax:.3e} rel-l2 {el2:.3e}   [worst {group} so far {WORST[group]:.3e}]")
    assert np.isfinite(got).all(), what
    assert emax <= bar and el2 <= bar, (what, emax, el2)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert diff.size == 0, (what, diff[:4], a.ravel()[diff[:4]], b.ravel()[diff[:4]])


def offset_view(x, off=5, extra=37):
    """x (B,T) as a view at column ``off`` of a (B, T+extra) leaf: row stride T+extra, base not 16-byte aligned."""
    B, T = x.shape
    wide = np.zeros((B, T + extra), np.float32)
    wide[:, off: off + T] = x
    leaf = dev(wide, True)
    view = leaf[:, off: off + T]
    assert view.data_ptr() % 16 != 0 and view.stride(0) == T + extra
    return leaf, view


def transposed(g):
    """g (B,T) with the values laid out T-major: strides (1, B)."""
    t = dev(np.asarray(g).T).t()
    assert t.shape == g.shape and (t.stride(1) != 1 or g.shape[0] == 1)
    return t


# ================================================================================================ LTI FIR
@functools.lru_cache(maxsize=None)
def lti_ref(case):
    ex, taps, gy = R.lti_inputs(*case)
    return (R.lti_fir(ex, taps, case[3]),) + R.lti_fir_grads(gy, ex, taps, case[3])


def run_lti(ex, taps, lead, gy, want=("ex", "taps")):
    """GF.lti_fir under autograd -> (y, g_ex or None, g_taps or None) as numpy."""
    from golf_amd import functional as GF

    x = ex if torch.is_tensor(ex) else dev(ex, "ex" in want)
    t = dev(taps, "taps" in want)
    g = gy if torch.is_tensor(gy) else dev(gy)
    y = GF.lti_fir(x, t, lead)
    ins = [v for v, k in ((x, "ex"), (t, "taps")) if k in want]
    grads = dict(zip([k for k in ("ex", "taps") if k in want], torch.autograd.grad(y, ins, g)))
    torch.cuda.synchronize()
    return host(y), host(grads["ex"]) if "ex" in grads else None, host(grads["taps"]) if "taps" in grads else None


@pytest.mark.parametrize("case", R.LTI_CASES + [R.LTI_LARGEST], ids=str)
def test_lti_fir_vs_reference(case):
    """| (3,253,4,0), (3,253,4,3)      | fewest taps, one sample past a tile
       | (2,1,8,0), (1,3,12,11)        | T < ntaps
       | (2,252,8,5)                   | exactly one tile
       | (2,961,252,100)               | one tap pass; second stretch of length 1: zero packed groups, the tail loop does it all
       | (2,962,252,0)                 | tail 2
       | (2,1923,264,{0,101,263})      | 2 passes x 3 stretches, tail 3
       | (2,2883,512,200)              | 3 passes x 4 stretches
       | (1,300,3836,1000)             | the largest tap count the 64 KiB of dynamic LDS admit"""
    ex, taps, gy = R.lti_inputs(*case)
    y, g_ex, g_taps = run_lti(ex, taps, case[3], gy)
    ry, rg_ex, rg_taps = lti_ref(case)
    check(y, ry, f"lti {case} y", R.FWD_BAR, "LTI")
    check(g_ex, rg_ex, f"lti {case} g_ex", R.GRAD_BAR, "LTI")
    check(g_taps, rg_taps, f"lti {case} g_taps", R.GRAD_BAR, "LTI")


def test_lti_oversize_is_refused_naming_lds():
    from golf_amd import _lib
    from golf_amd import functional as GF

    ex = torch.zeros(1, 300, device="cuda")
    with pytest.raises(_lib.GolfError, match="bad argument -3: .*LDS.*3836"):     # GOLF_EUNSUPPORTED, the largest size named
        GF.lti_fir(ex, torch.zeros(3840, device="cuda"), 1000)
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [(2, 1923, 264, 101), (3, 253, 4, 3), (1, 3, 12, 11)], ids=str)
def test_lti_reversed_taps_through_the_abi(case):
    """golf_lti_fir_f32 with -n taps applies them in reverse order: the same operations in the same order as the call with
    taps.flip(0) and +n, so the same bits."""
    from golf_amd import _lib

    lib = _lib.load()
    B, T, n, lead = case
    ex, taps, _ = R.lti_inputs(*case)
    x, t = dev(ex), dev(taps)
    tf = t.flip(0).contiguous()
    out = []
    for tp, cnt in ((t, -n), (tf, n)):
        y = torch.full((B, T), float("nan"), device="cuda")
        _lib.check(lib.golf_lti_fir_f32(x.data_ptr(), x.stride(0), tp.data_ptr(), cnt, lead, y.data_ptr(), y.stride(0), B, T,
                                        _lib.stream_ptr()), "golf_lti_fir_f32")
        torch.cuda.synchronize()
        out.append(host(y))
    same_bits(out[0], out[1], f"reversed taps {case}")
    check(out[0], R.lti_fir(ex, taps[::-1], lead), f"reversed taps {case}", R.FWD_BAR, "LTI")


@pytest.mark.parametrize("case", [(2, 1923, 264, 101), (3, 253, 4, 0)], ids=str)
def test_lti_strided_inputs_give_the_same_bits(case):
    B, T, n, lead = case
    ex, taps, gy = R.lti_inputs(*case)
    y, g_ex, g_taps = run_lti(ex, taps, lead, gy)
    from golf_amd import functional as GF

    leaf, view = offset_view(ex)
    t = dev(taps, True)
    ys = GF.lti_fir(view, t, lead)
    g_leaf, g_t = torch.autograd.grad(ys, (leaf, t), transposed(gy))
    torch.cuda.synchronize()
    same_bits(host(ys), y, "strided y")
    same_bits(host(g_leaf)[:, 5: 5 + T], g_ex, "strided g_ex")
    same_bits(host(g_t), g_taps, "strided g_taps")
    outside = host(g_leaf).copy()
    outside[:, 5: 5 + T] = 0
    assert np.all(outside == 0), "gradient outside the view"


def test_lti_partial_gradients_give_the_same_bits():
    case = (2, 1923, 264, 101)
    ex, taps, gy = R.lti_inputs(*case)
    y, g_ex, g_taps = run_lti(ex, taps, case[3], gy)
    y1, g_ex1, none = run_lti(ex, taps, case[3], gy, want=("ex",))
    assert none is None
    y2, none, g_taps2 = run_lti(ex, taps, case[3], gy, want=("taps",))
    assert none is None
    for a, b, what in ((y1, y, "y (ex only)"), (y2, y, "y (taps only)"), (g_ex1, g_ex, "g_ex"), (g_taps2, g_taps, "g_taps")):
        same_bits(a, b, what)


def test_lti_rows_do_not_depend_on_the_batch():
    """B = 5 rows of 3 tiles: 15 units, not a multiple of the 4 waves of a workgroup; every row equals its own B = 1 call."""
    B, T, n, lead = R.LTI_BATCH
    assert (B * -(-T // 252)) % 4 != 0
    ex, taps, gy = R.lti_inputs(B, T, n, lead)
    y, g_ex, g_taps = run_lti(ex, taps, lead, gy)
    for name, got, ref, bar in zip(("y", "g_ex", "g_taps"), (y, g_ex, g_taps), lti_ref(R.LTI_BATCH), (R.FWD_BAR, R.GRAD_BAR, R.GRAD_BAR)):
        check(got, ref, f"B=5 {name}", bar, "LTI")
    for b in range(B):
        yb, gb, _ = run_lti(ex[b: b + 1], taps, lead, gy[b: b + 1])
        same_bits(yb[0], y[b], f"row {b} y")
        same_bits(gb[0], g_ex[b], f"row {b} g_ex")


@pytest.mark.parametrize("case", [(2, 1923, 264, 101), (3, 253, 4, 3), (2, 1, 8, 0)], ids=str)
def test_lti_writes_every_output_and_nothing_else(case):
    """NaN-filled y (row stride T + 11) and g_taps through the C ABI: all of [0,T) and every tap finite, the padding columns
    still NaN."""
    from golf_amd import _lib

    lib = _lib.load()
    B, T, n, lead = case
    ex, taps, gy = R.lti_inputs(*case)
    x, t, g = dev(ex), dev(taps), dev(gy)
    y = torch.full((B, T + 11), float("nan"), device="cuda")
    _lib.check(lib.golf_lti_fir_f32(x.data_ptr(), x.stride(0), t.data_ptr(), n, lead, y.data_ptr(), y.stride(0), B, T,
                                    _lib.stream_ptr()), "golf_lti_fir_f32")
    g_taps = torch.full((n,), float("nan"), device="cuda")
    nbytes = lib.golf_lti_fir_taps_grad_workspace_bytes(B, T, n)
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda").fill_(0xFF)
    _lib.check(lib.golf_lti_fir_taps_grad_f32(g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), g_taps.data_ptr(), n, lead,
                                              B, T, ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "golf_lti_fir_taps_grad_f32")
    torch.cuda.synchronize()
    yh = host(y)
    assert np.isfinite(yh[:, :T]).all() and np.isnan(yh[:, T:]).all()
    ry, _, rg_taps = lti_ref(case)
    check(yh[:, :T], ry, f"abi {case} y", R.FWD_BAR, "LTI")
    check(host(g_taps), rg_taps, f"abi {case} g_taps", R.GRAD_BAR, "LTI")


# ================================================================================================ frame FIR
@functools.lru_cache(maxsize=None)
def frames_ref(cid, causal):
    c = R.frames_inputs(cid, causal)
    y = R.frames_fir(c["ex"], c["kern"], c["hop"], causal, c["frame0"])
    if c["hop"] % 4:
        return y, None, None
    return (y,) + R.frames_fir_grads(c["gy"], c["ex"], c["kern"], c["hop"], causal, c["frame0"])


def frames_apply(c, ex, kern):
    """GF.ltv_fir_frames / _causal where they take the case; _FIRFrames.apply (rows padded to a multiple of 16, as the
    wrappers pad them) for frame0 > 0 and for more causal excitation than kernels, which the causal wrapper refuses."""
    from golf_amd import functional as GF

    N, hop, F, f0, causal = c["N"], c["hop"], c["F"], c["frame0"], c["causal"]
    if f0 == 0 and not (causal and c["T"] // hop > F):
        return (GF.ltv_fir_frames_causal if causal else GF.ltv_fir_frames)(ex, kern, hop)
    KS = (N + 15) // 16 * 16
    rows = torch.nn.functional.pad(kern.reshape(-1, N), (0, KS - N))
    return GF._FIRFrames.apply(ex, rows, F, N, hop, f0, causal)


def run_frames(c, ex=None, gy=None):
    """-> (y, g_ex, g_kern (B,F,N)) as numpy, through autograd; ``ex`` = (leaf, view) and ``gy`` may be given strided."""
    leaf, x = ex if ex is not None else (None, dev(c["ex"], True))
    k = dev(c["kern"], True)
    y = frames_apply(c, x, k)
    assert y.shape == (c["B"], c["nfr"] * c["hop"])
    g_x, g_k = torch.autograd.grad(y, (leaf if leaf is not None else x, k), gy if gy is not None else dev(c["gy"]))
    torch.cuda.synchronize()
    return host(y), host(g_x), host(g_k)


def abi_frames(c):
    """Forward and backward through the C ABI into NaN-filled buffers with padded rows: y (stride nfr*hop + 9), g_ex
    (stride T + 7), g_kern (B*F, KS).  -> the three whole buffers as numpy."""
    from golf_amd import _lib

    lib = _lib.load()
    N, hop, F, f0, B, T, nfr = (c[k] for k in ("N", "hop", "F", "frame0", "B", "T", "nfr"))
    name = "golf_ltv_fir_frames_causal" if c["causal"] else "golf_ltv_fir_frames"
    KS = (N + 15) // 16 * 16
    x, g = dev(c["ex"]), dev(c["gy"])
    rows = dev(np.pad(c["kern"].reshape(B * F, N), ((0, 0), (0, KS - N))))
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")   # noqa: E731
    y, g_ex, g_kern = nan(B, nfr * hop + 9), nan(B, T + 7), nan(B * F, KS)
    _lib.check(getattr(lib, name + "_fwd_f32")(x.data_ptr(), x.stride(0), rows.data_ptr(), KS, y.data_ptr(), y.stride(0), B, T,
                                               F, N, hop, f0, _lib.stream_ptr()), name + "_fwd_f32")
    _lib.check(getattr(lib, name + "_bwd_f32")(g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), rows.data_ptr(), KS,
                                               g_ex.data_ptr(), g_ex.stride(0), g_kern.data_ptr(), B, T, F, N, hop, f0,
                                               _lib.stream_ptr()), name + "_bwd_f32")
    torch.cuda.synchronize()
    return host(y), host(g_ex), host(g_kern).reshape(B, F, KS)


def group(causal):
    return "frames causal" if causal else "frames zero-phase"


def check_frames(c, cid, got):
    causal = c["causal"]
    for name, g, r, bar in zip(("y", "g_ex", "g_kern"), got, frames_ref(cid, causal), (R.FWD_BAR, R.GRAD_BAR, R.GRAD_BAR)):
        check(g, r, f"frames {cid} causal={causal} {name}", bar, group(causal))


SHAPE_IDS = [cid for cid in R.FRAMES_CASES if cid.split("-")[0] in ("small", "mod4", "pass", "tile", "many", "largest")]


@pytest.mark.parametrize("causal", [False, True], ids=["zero-phase", "causal"])
@pytest.mark.parametrize("cid", SHAPE_IDS)
def test_frames_vs_reference(cid, causal):
    """small: N in {5,7} x hop in {4,48} (hop 4 is the smallest the backward takes); mod4: every remainder of N modulo 4;
    pass: N around the 252-tap pass of bwd_kern (rows of (N+15)//16*16); tile: hop around the 252-output tile (forward
    passes 1,1,2,2,3; the bwd_ex tile is hop, then 252); many-frames: ~14 frames reach one bwd_ex tile; largest: the last
    N (forward) and hop (backward) the 64 KiB of dynamic LDS admit."""
    c = R.frames_inputs(cid, causal)
    check_frames(c, cid, run_frames(c))


@pytest.mark.parametrize("causal", [False, True], ids=["zero-phase", "causal"])
@pytest.mark.parametrize("cid", ["one-frame", "long-tail", "unused-rows", "frame0-0", "frame0-1", "frame0-2"])
def test_frames_write_every_output_and_nothing_else(cid, causal):
    """Through the C ABI into NaN-filled buffers.  one-frame: the smallest legal T; long-tail: T far past the last frame's
    reach, the tail of g_ex exactly 0 and written; unused-rows: F = nfr + 3; frame0: output frame f uses row f + frame0.
    In all of them: g_kern rows below frame0 and from frame0 + nfr on exactly 0, the padding taps [N, KS) exactly 0, the
    padding columns of y and g_ex untouched."""
    c = R.frames_inputs(cid, causal)
    N, hop, F, f0, T, nfr = (c[k] for k in ("N", "hop", "F", "frame0", "T", "nfr"))
    y, g_ex, g_kern = abi_frames(c)
    assert np.isnan(y[:, nfr * hop:]).all() and np.isnan(g_ex[:, T:]).all(), "wrote past a row"
    assert np.isfinite(y[:, :nfr * hop]).all() and np.isfinite(g_ex[:, :T]).all() and np.isfinite(g_kern).all(), "unwritten"
    check_frames(c, cid, (y[:, :nfr * hop], g_ex[:, :T], g_kern[:, :, :N]))
    assert np.all(g_kern[:, :, N:] == 0), "padding taps"
    assert np.all(g_kern[:, :f0] == 0) and np.all(g_kern[:, f0 + nfr:] == 0), "unused kernel rows"
    assert np.any(g_kern[:, f0] != 0) and np.any(g_kern[:, f0 + nfr - 1] != 0)
    assert np.all(g_ex[:, R.frames_reach(c): T] == 0), "excitation no frame reads"
    if cid in ("one-frame", "unused-rows") or f0 > 0:       # the autograd path agrees with the ABI bit for bit
        ya, ga_ex, ga_kern = run_frames(c)
        same_bits(ya, y[:, :nfr * hop], "autograd y")
        same_bits(ga_ex, g_ex[:, :T], "autograd g_ex")
        same_bits(ga_kern, g_kern[:, :, :N], "autograd g_kern")


@pytest.mark.parametrize("causal", [False, True], ids=["zero-phase", "causal"])
@pytest.mark.parametrize("hop", R.FRAMES_ODD_HOPS)
def test_frames_hops_that_are_no_multiple_of_4(hop, causal):
    from golf_amd import _lib

    cid = f"odd-hop{hop}"
    c = R.frames_inputs(cid, causal)
    x, k = dev(c["ex"], True), dev(c["kern"], True)
    y = frames_apply(c, x, k)
    torch.cuda.synchronize()
    check(host(y), frames_ref(cid, causal)[0], f"frames {cid} causal={causal} y", R.FWD_BAR, group(causal))
    with pytest.raises(_lib.GolfError, match=f"bad argument -3: .*hop={hop} must be a multiple of 4"):   # GOLF_EUNSUPPORTED
        torch.autograd.grad(y, (x, k), dev(c["gy"]))
    torch.cuda.synchronize()


@pytest.mark.parametrize("causal", [False, True], ids=["zero-phase", "causal"])
@pytest.mark.parametrize("cid", ["mod4-N51", "tile-hop504", "frame0-1"])
def test_frames_strided_inputs_give_the_same_bits(cid, causal):
    c = R.frames_inputs(cid, causal)
    y, g_ex, g_kern = run_frames(c)
    ys, g_leaf, g_ks = run_frames(c, ex=offset_view(c["ex"]), gy=transposed(c["gy"]))
    T = c["T"]
    same_bits(ys, y, "strided y")
    same_bits(g_leaf[:, 5: 5 + T], g_ex, "strided g_ex")
    same_bits(g_ks, g_kern, "strided g_kern")
    g_leaf[:, 5: 5 + T] = 0
    assert np.all(g_leaf == 0), "gradient outside the view"


@pytest.mark.parametrize("causal", [False, True], ids=["zero-phase", "causal"])
def test_frames_oversize_is_refused_naming_lds(causal):
    """N = 3840 in the forward, and N = 3837, which rounds up to 3840 packed taps; hop = 3840 in the backward (its forward,
    16 passes, runs)."""
    from golf_amd import _lib
    from golf_amd import functional as GF

    for N in (3837, 3840):
        with pytest.raises(_lib.GolfError, match="bad argument -3: .*LDS.*3836"):
            GF._FIRFrames.apply(torch.zeros(1, 300, device="cuda"), torch.zeros(1, 3840, device="cuda"), 1, N, 8, 0, causal)
    x, k = torch.zeros(1, 3840 + 300, device="cuda", requires_grad=True), torch.zeros(1, 16, device="cuda", requires_grad=True)
    y = GF._FIRFrames.apply(x, k, 1, 8, 3840, 0, causal)
    assert y.shape == (1, 3840)
    with pytest.raises(_lib.GolfError, match="bad argument -3: .*LDS.*3836"):
        torch.autograd.grad(y, (x, k), torch.ones_like(y))
    torch.cuda.synchronize()


# ================================================================================================ decimator
@functools.lru_cache(maxsize=None)
def decim_ref(case):
    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    return R.decimate(x, taps, os_), R.decimate_adjoint(g, taps, os_, N)


def run_decimate(x, taps, os_, g=None):
    from golf_amd import functional as GF

    xt = x if torch.is_tensor(x) else dev(x, g is not None)
    out = GF.decimate_fir(xt, dev(taps), os_)
    gx = None
    if g is not None:
        (gx,) = torch.autograd.grad(out, xt, dev(g))
    torch.cuda.synchronize()
    return host(out), None if gx is None else host(gx)


@pytest.mark.parametrize("case", R.DECIM_CASES, ids=str)
def test_decimator_vs_reference(case):
    """os in {2,3,4} with the designed taps (65, 97, 129) and os in {5,8} with random odd K in {1,3,31,255}, at N with Tout in
    {1, 2, 1024, 1025} (the 1024-output tile) and N in {1, os, os+1}."""
    os_, K, N = case
    x, taps, _ = R.decim_inputs(*case)
    out, _ = run_decimate(x, taps, os_)
    assert out.shape == (x.shape[0], (N - 1) // os_ + 1)
    check(out, decim_ref(case)[0], f"decimate {case}", R.FWD_BAR, "decimator")
    if K == 1:
        same_bits(out, taps[0] * x[:, ::os_], f"decimate {case}: one tap")


@pytest.mark.parametrize("case", R.DECIM_ADJ_CASES, ids=str)
def test_decimator_adjoint_vs_reference(case):
    """os in {2,3,5}: osc_decimate_T_kernel; os = 4: osc_decimate_T4_kernel.  On the GPU's own results the dot-product
    identity <A x, g> = <x, A' g> holds within 1e-5 of |A x| |g| (each side is within its bar of the exact value in L2,
    and Cauchy-Schwarz turns that into this scale)."""
    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    out, gx = run_decimate(x, taps, os_, g)
    ry, rgx = decim_ref(case)
    check(out, ry, f"decimate {case}", R.FWD_BAR, "decimator")
    check(gx, rgx, f"decimate adjoint {case}", R.GRAD_BAR, "decimator")
    lhs = (out.astype(np.float64) * g).sum()
    rhs = (x.astype(np.float64) * gx).sum()
    scale = np.linalg.norm(out.astype(np.float64)) * np.linalg.norm(g.astype(np.float64))
    print(f"decimate {case}: <Ax,g> {lhs:.9e} <x,A'g> {rhs:.9e} |difference| / (|Ax||g|) {abs(lhs - rhs) / scale:.2e}")
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_decimator_fill_paths_give_the_same_bits():
    """os = 4, N = 12000: three tiles, the middle one interior.  A 16-byte aligned base with a row stride divisible by 4
    takes the vec4 fill there; the same data one float further with row stride N + 1 takes the bounds-checked fill."""
    os_, K, N = R.DECIM_FILL
    x, taps, _ = R.decim_inputs(os_, K, N)
    B = x.shape[0]
    aligned = dev(x)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(0) % 4 == 0
    flat = torch.zeros(B * (N + 1) + 1, device="cuda")
    shifted = flat[1:].view(B, N + 1)[:, :N]
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 16 == 4 and shifted.stride(0) == N + 1
    a, _ = run_decimate(aligned, taps, os_)
    s, _ = run_decimate(shifted, taps, os_)
    same_bits(a, s, "vec4 fill vs bounds-checked fill")
    check(a, R.decimate(x, taps, os_), "decimate os 4 N 12000 (vec4 fill)", R.FWD_BAR, "decimator")
    check(s, R.decimate(x, taps, os_), "decimate os 4 N 12000 (checked fill)", R.FWD_BAR, "decimator")


@pytest.mark.parametrize("case", [(4, None, 4097), (5, 31, 5121), (3, None, 4)], ids=str)
def test_decimator_strides_and_untouched_padding_through_the_abi(case):
    """Strided x and g_out, NaN-filled out (row stride Tout + 5) and g_x: every element written, the padding still NaN."""
    from golf_amd import _lib

    lib = _lib.load()
    os_, K, N = case
    x, taps, g = R.decim_inputs(*case)
    B, Tout = g.shape
    K = taps.shape[0]
    _, xv = offset_view(x)
    _, gv = offset_view(g, off=3, extra=9)
    t = dev(taps)
    out = torch.full((B, Tout + 5), float("nan"), device="cuda")
    g_x = torch.full((B, N), float("nan"), device="cuda")
    _lib.check(lib.golf_decimate_fir_f32(xv.data_ptr(), xv.stride(0), N, t.data_ptr(), K, os_, out.data_ptr(), out.stride(0), B,
                                         Tout, _lib.stream_ptr()), "golf_decimate_fir_f32")
    _lib.check(lib.golf_decimate_fir_adj_f32(gv.data_ptr(), gv.stride(0), Tout, t.data_ptr(), K, os_, g_x.data_ptr(), N, B,
                                             _lib.stream_ptr()), "golf_decimate_fir_adj_f32")
    torch.cuda.synchronize()
    oh = host(out)
    assert np.isnan(oh[:, Tout:]).all() and np.isfinite(oh[:, :Tout]).all()
    ry, rgx = decim_ref(case)
    check(oh[:, :Tout], ry, f"abi decimate {case}", R.FWD_BAR, "decimator")
    check(host(g_x), rgx, f"abi decimate adjoint {case}", R.GRAD_BAR, "decimator")
    a, ga = run_decimate(x, taps, os_, g)
    same_bits(oh[:, :Tout], a, "strided vs contiguous out")
    same_bits(host(g_x), ga, "strided vs contiguous g_x")


def test_decimator_refusals():
    """All of them on the host, before any launch."""
    from golf_amd import _lib
    from golf_amd import functional as GF

    lib = _lib.load()
    x = torch.zeros(2, 100, device="cuda")
    odd, even = torch.zeros(31, device="cuda"), torch.zeros(30, device="cuda")
    for taps, os_ in ((even, 4), (odd, 1), (odd, 65)):
        with pytest.raises(_lib.GolfError):
            GF.decimate_fir(x, taps, os_)
    out = torch.zeros(2, 100, device="cuda")
    for bad_tout in (24, 26):                            # (100 - 1) // 4 + 1 = 25
        with pytest.raises(_lib.GolfError, match="Tout"):
            _lib.check(lib.golf_decimate_fir_f32(x.data_ptr(), x.stride(0), 100, odd.data_ptr(), 31, 4, out.data_ptr(),
                                                 out.stride(0), 2, bad_tout, _lib.stream_ptr()), "golf_decimate_fir_f32")
        with pytest.raises(_lib.GolfError, match="Tout"):
            _lib.check(lib.golf_decimate_fir_adj_f32(out.data_ptr(), out.stride(0), bad_tout, odd.data_ptr(), 31, 4,
                                                     x.data_ptr(), 100, 2, _lib.stream_ptr()), "golf_decimate_fir_adj_f32")
    with pytest.raises(_lib.GolfError, match="LDS") as e:
        GF.decimate_fir(x, torch.zeros(513, device="cuda"), 16)
    assert "bad argument -3" in str(e.value)             # GOLF_EUNSUPPORTED, not a hipError
    torch.cuda.synchronize()


def test_zz_worst_values_per_group():
    """Not a check: the worst rel-max of every group, for the record (-s shows it)."""
    for g, v in sorted(WORST.items()):
        print(f"worst rel-max, {g}: {v:.3e}")
