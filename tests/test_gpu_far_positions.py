"""The block-by-block entries far into a stream.  They take int64 positions and promise them up to 2^62 (2^40 samples for the
harmonic bank, 2^31 frames for the fixed-lag path search); a 24 kHz stream passes sample 2^31 after 25 hours, and the other
stream tests stop at a few thousand samples, where an ``(int)t`` or an ``int`` product in a kernel or a launcher is invisible.

Invariant: an entry's result depends on its positions only through their differences, and a ring slot on the position modulo
the ring size.  So the same buffers declared D frames later give the same bits: every test runs a call (or a chain of calls)
from the middle of a short stream -- nothing reads before sample 0, no frame reflects at the stream's start -- and its twin
with every position shifted, on the same input buffers and on a copy of the same carried state, and compares the outputs and
the state afterwards with ``torch.equal``.  The base calls are tied to the one-shot results here where that is one line;
tests/test_gpu_residual.py, test_gpu_hna_stream.py, test_gpu_env_stream.py, test_gpu_stream_stft.py, test_gpu_stream_ff.py,
test_gpu_stream.py, test_gpu_stream_hpn.py and test_gpu_f0_stream.py hold them to their references.

Two shifts per entry: one puts the samples in [2^31, 2^32) (a signed 32-bit cast), one above 2^40 (an unsigned one; just
under 2^40 for the harmonic bank, which caps there; the path search refuses frame 2^31 and has the one shift just below).
No shift is a multiple of 2^32 samples: a truncation to 32 bits would then alias onto the base position and pass.

Periods the shifts respect: the carried-frame rings of the two frame filters hold frame f in slot f % S, S = ceil(W / hop)
- 1 (csrc/stream_plan.h), and their base chains start at frame S or later, where every slot holds a frame that exists (the
frames before 0 do not, and the overlap-add leaves them out of its norm); the path search keeps its carry at f % lag and its LDS rings at f % VS_RING = 2048
(csrc/f0_viterbi_stream.hip); an amplitude or tscale track of the harmonic bank moves by D * P / hop rows, a whole number."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WRAP = 1 << 32


def dev(a):
    return a if isinstance(a, torch.Tensor) else torch.tensor(a).cuda()


def far_shifts(unit, period=1):
    """Two shifts in steps of ``unit`` samples, multiples of ``period`` steps: the first at least 2^31 + 12345 samples, the
    second at least 2^40 + 12345."""
    return [-(-(lo + 12345) // (unit * period)) * period for lo in (1 << 31, 1 << 40)]


def check_shifts(shifts, lo, hi):
    """``shifts`` in samples, the base call's positions in [lo, hi): the first lands in [2^31, 2^32), the second above 2^40,
    and neither is a multiple of 2^32, which a 32-bit truncation would map onto the base position."""
    near, far = shifts
    assert 1 << 31 <= near + lo and near + hi <= WRAP
    assert far + lo > 1 << 40
    assert near % WRAP and far % WRAP


def same(a, b):
    a, b = (a if isinstance(a, (tuple, list)) else (a,)), (b if isinstance(b, (tuple, list)) else (b,))
    return len(a) == len(b) and all(u.shape == v.shape and u.numel() > 0 and torch.equal(u, v) for u, v in zip(a, b))


# ---- the analysis entries: one call at a position ---------------------------------------------------------------------------
@pytest.mark.parametrize("last", [False, True])
def test_ltv_residual_stream(last):
    import residual_ref as R
    from golf_amd import functional as GF

    B, F, M, hop, T = 2, 12, 22, 16, 177
    x, gain, a = (dev(t) for t in R.inputs(B, F, M, T, 5))
    # t_first >= M: every tap of the first sample exists; without ``last`` the frame after the last sample is in the buffer
    t_first, n_out, x_t0, x_end, fr_first, fr_end = (60, 117, 30, 177, 2, 12) if last else (60, 70, 30, 150, 2, 11)
    assert t_first - M >= x_t0 > 0 and fr_first > 0

    def call(D):
        return GF.ltv_residual_stream(x[:, x_t0:x_end], gain[:, fr_first:fr_end], a[:, fr_first:fr_end], x_t0 + D * hop,
                                      fr_first + D, t_first + D * hop, n_out, last, hop)

    shifts = far_shifts(hop)
    check_shifts([D * hop for D in shifts], x_t0, x_end)
    base = call(0)
    assert torch.equal(base, GF.ltv_residual(x, gain, a, hop)[:, t_first:t_first + n_out])
    for D in shifts:
        assert same(call(D), base), D


@pytest.mark.parametrize("last", [False, True])
def test_harmonic_analysis_stream(last):
    from golf_amd import functional as GF
    from test_gpu_hna_stream import case, one_shot

    x, f0, kw = case("small")
    hop, Lmax = kw["hop"], max(kw["max_window"], kw["unvoiced_window"])
    (T, F) = x.shape[1], f0.shape[1]
    f_first, n, x_t0, x_end, f0_first, f0_end = (30, 14, 400, T, 28, F) if last else (10, 10, 90, 380, 8, 22)
    assert 0 < x_t0 <= f_first * hop - Lmax // 2 and 0 < f0_first < f_first and f_first + n == (F if last else 20)
    assert (f0[0, 10:20] > 0).all() and f0[0, 9] == 0 and f0[0, 20] == 0   # chirps from both neighbours, and from one
    more = {k: v for k, v in kw.items() if k not in ("sample_rate", "hop", "K")}

    def call(D):
        return GF.harmonic_analysis_stream(x[:, x_t0:x_end], f0[:, f0_first:f0_end], x_t0 + D * hop, f_first + D, f0_first + D,
                                           n, last, kw["sample_rate"], hop, kw["K"], return_phases=True, **more)

    shifts = far_shifts(hop)
    check_shifts([D * hop for D in shifts], x_t0, x_end)
    base = call(0)
    assert len(base) == 3 and same(base, [r[:, f_first:f_first + n] for r in one_shot(x, f0, kw)])
    for D in shifts:
        assert same(call(D), base), D


@pytest.mark.parametrize("last", [False, True])
def test_spectral_envelope_stream(last):
    from golf_amd import functional as GF
    from test_gpu_env_stream import hwmax_of, one_shot

    x, f0, kw, ref = one_shot("mixed")   # voiced, unvoiced, NaN and negative f0 side by side
    hop, hw = kw["hop"], hwmax_of(kw)
    (T, F) = x.shape[1], f0.shape[1]
    f_first, n = (7, 5) if last else (3, 4)
    x_t0, x_end = f_first * hop - hw - 7, T if last else (f_first + n - 1) * hop + hw + 1 + 5
    f0_first, f0_end = f_first - 1, F if last else f_first + n + 1
    assert x_t0 > 0 and x_end <= T and f_first + n == (F if last else 7)
    more = {k: v for k, v in kw.items() if k not in ("sample_rate", "hop")}

    def call(D):
        return GF.spectral_envelope_stream(x[:, x_t0:x_end], f0[:, f0_first:f0_end], x_t0 + D * hop, f_first + D, f0_first + D,
                                           n, last, kw["sample_rate"], hop, **more)

    shifts = far_shifts(hop)
    check_shifts([D * hop for D in shifts], x_t0, x_end)
    base = call(0)
    assert len(base) == 2 and same(base, [r[:, f_first:f_first + n] for r in ref])
    for D in shifts:
        assert same(call(D), base), D


# ---- the frame filters: a chain of calls over a carried ring ---------------------------------------------------------------
def stft_chain(x, H, window, hop, bounds, carry, D, f_start, n_start):
    """Calls over the frames [f_start, bounds[0]), [bounds[0], bounds[1]), ..., each given the samples its frames read, every
    position declared D frames later; the call that reaches the last frame ends the utterance.  -> (outputs, carry)."""
    from golf_amd import functional as GF

    T, frames, pad = x.shape[1], H.shape[1], window.numel() // 2
    outs, f0, n0 = [], f_start, n_start
    for f1 in bounds:
        x_lo = f0 * hop - pad - 1   # (the last frame's reflection reads one sample before its own span)
        assert x_lo >= 0 or f0 == 0
        x_lo = max(x_lo, 0)
        if f1 == frames:
            xs, ny, end = x[:, x_lo:], hop * (frames - 1) - n0, dict(x_end=T + D * hop, frames_end=frames + D)
        else:
            xs, ny, end = x[:, x_lo:(f1 - 1) * hop + pad + 1], f1 * hop - pad - n0, {}
        y, carry = GF.stft_filter_stream(xs, H[:, f0:f1], window, hop, carry, x0=x_lo + D * hop, h0=f0 + D, f0=f0 + D,
                                         nf=f1 - f0, n0=n0 + D * hop, ny=ny, **end)
        outs.append(y)
        f0, n0 = f1, n0 + ny
    return outs, carry


@pytest.mark.parametrize("n,hop,kind", [(64, 24, "complex"), (1024, 240, "real")])
def test_stft_filter_stream(n, hop, kind):
    from golf_amd import functional as GF

    B, frames, pad = 2, 13, n // 2
    T = (frames - 1) * hop + 5
    S = -(-n // hop) - 1
    gen = torch.Generator().manual_seed(n + hop)
    x = torch.randn(B, T, generator=gen).cuda()
    H = torch.rand(B, frames, pad + 1, generator=gen) + 0.5
    H = (torch.complex(H, 0.2 * torch.randn(B, frames, pad + 1, generator=gen)) if kind == "complex" else H).cuda()
    window = torch.hann_window(n).cuda()
    # The chain starts at a frame whose samples, and the one before them, lie right of sample 0, and not before frame S: the
    # frames before 0 do not exist and the overlap-add leaves them out of its norm, while the twin's frames D - 1, D - 2, ..
    # do exist.  (Measured with a start at frame 3 < S = 4 at n 1024, hop 240: the first samples differ by 1e-3.)
    fa = max(-(-(pad + 1) // hop), S)
    assert fa * hop - pad - 1 >= 0 and fa - S >= 0
    head, carry0 = stft_chain(x, H, window, hop, [fa], None, 0, 0, 0)   # an ordinary chain from 0 leaves the carry behind
    carry0 = carry0.clone()
    bounds, n_start = [fa + 3, fa + 6, frames], fa * hop - pad
    assert len(bounds) >= 3 and fa + 6 < frames and S >= 2
    shifts = far_shifts(hop, S)
    assert all(D % S == 0 for D in shifts)   # ring slots are f % S
    check_shifts([D * hop for D in shifts], fa * hop - pad - 1, T)
    base, carry = stft_chain(x, H, window, hop, bounds, carry0.clone(), 0, fa, n_start)
    assert torch.equal(torch.cat(head + base, 1), GF.stft_filter_frames(x, H, window, hop))
    assert not torch.equal(carry, carry0)
    for D in shifts:
        got, moved = stft_chain(x, H, window, hop, bounds, carry0.clone(), D, fa, n_start)
        assert same(got, base) and torch.equal(moved, carry), D


def ff_chain(ex, gain, a, win, hop, bounds, carry, D, f_start, n_start):
    """tests/test_gpu_stream_ff.py's _stream_filter from a frame on, every position declared D frames later."""
    from golf_amd import functional as GF

    F, W = a.shape[1], win.numel()
    Tx, nfr, Ty = GF.ff_output_length(ex.shape[1], F, hop, W)
    pad = W // 2
    seg = lambda t, fin: min(t // hop, F - 2) if fin else t // hop
    outs, f0, n0 = [], f_start, n_start
    for f1 in bounds:
        fin = f1 == nfr
        ny = (Ty if fin else f1 * hop - pad) - n0
        tlo, thi = max(0, f0 * hop - pad), (f1 - 1) * hop - pad + W
        thi = min(thi, Tx) if fin else thi
        g_lo, g_hi = seg(tlo, fin), seg(thi - 1, fin) + 2
        y, carry = GF.lti_frames_ola_stream(ex[:, tlo:thi], gain[:, g_lo:g_hi], a[:, f0:f1], win, hop, carry,
                                            x0=tlo + D * hop, g0=g_lo + D, a0=f0 + D, f0=f0 + D, nf=f1 - f0, n0=n0 + D * hop,
                                            ny=ny, x_end=Tx + D * hop if fin else -1, g_end=F + D if fin else -1)
        outs.append(y)
        f0, n0 = f1, n0 + ny
    return outs, carry


# the recipe's shape runs the block recursion (ring 24, W % 32 == 0, hop % 4 == 0); hop 10 is no multiple of 4: the plain ring
@pytest.mark.parametrize("M,hop,W", [(22, 240, 960), (6, 10, 30)])
def test_lti_frames_ola_stream(M, hop, W):
    from golf_amd import functional as GF
    from test_gpu_stream_ff import _stream_filter

    B, F, pad = 2, 14, W // 2
    S = -(-W // hop) - 1
    gen = torch.Generator().manual_seed(M + hop)
    a = GF.rc2lpc((0.5 * torch.tanh(torch.randn(B, F, M, generator=gen))).cuda())
    gain = torch.exp(0.1 * torch.randn(B, F, generator=gen)).cuda()
    ex = torch.randn(B, (F - 1) * hop + 1, generator=gen).cuda()
    win = torch.hann_window(W).cuda()
    nfr = GF.ff_output_length(ex.shape[1], F, hop, W)[1]
    fa = max(-(-pad // hop) + 1, S)   # past the first frame that starts right of sample 0, with every ring slot in use
    assert (fa - 1) * hop - pad >= 0 and fa - S >= 0 and nfr == F
    head, carry0 = ff_chain(ex, gain, a, win, hop, [fa], None, 0, 0, 0)   # an ordinary chain from 0 leaves the carry behind
    carry0 = carry0.clone()
    bounds, n_start = [fa + 3, fa + 6, nfr], fa * hop - pad
    assert fa + 6 <= 12 < nfr
    shifts = far_shifts(hop, S)
    assert all(D % S == 0 for D in shifts)   # ring slots are f % S
    check_shifts([D * hop for D in shifts], fa * hop - pad, ex.shape[1])
    base, carry = ff_chain(ex, gain, a, win, hop, bounds, carry0.clone(), 0, fa, n_start)
    assert torch.equal(torch.cat(head + base, 1), _stream_filter(ex, gain, a, win, hop, []))
    assert not torch.equal(carry, carry0)
    for D in shifts:
        got, moved = ff_chain(ex, gain, a, win, hop, bounds, carry0.clone(), D, fa, n_start)
        assert same(got, base) and torch.equal(moved, carry), D


# ---- the oscillators: a carried Q0.64 phase ---------------------------------------------------------------------------------
@pytest.mark.parametrize("final_point", [False, True])
@pytest.mark.parametrize("L", [256, 100])   # the table's column by a shift, and by a product
def test_glottal_osc_stream(L, final_point):
    from golf_amd import functional as GF

    B, phase_hop, os, w_hop = 2, 3, 4, 40
    P, hop_t = phase_hop * os, w_hop * os
    gen = torch.Generator().manual_seed(L)
    phase = (0.004 + 0.004 * torch.rand(B, 200, generator=gen)).cuda()
    wsel = torch.rand(B, 20, generator=gen).cuda()
    table = torch.randn(16, L, generator=gen).cuda()
    acc0 = torch.randint(-2 ** 62, 2 ** 62, (B,), generator=gen).cuda()
    j, nseg = 50, 120
    rows = slice(j * P // hop_t - 1, (j + nseg) * P // hop_t + 2)
    assert rows.start == 2 and rows.stop <= wsel.shape[1]

    def call(m):
        acc = acc0.clone()
        out = GF.glottal_osc_stream(phase[:, j:j + nseg + 1], j + m * w_hop, nseg, final_point, phase_hop, os, wsel[:, rows],
                                    rows.start + m * phase_hop, w_hop, table, True, acc, want_wrapped=True)
        return (*out, acc)

    shifts = far_shifts(w_hop * P)   # m table-select rows of the coarse track: m w_hop coarse samples, m w_hop P fine ones
    check_shifts([m * w_hop * P for m in shifts], j * P, (j + nseg) * P + 1)
    base = call(0)
    assert base[0].shape == (B, nseg * P + final_point) and not torch.equal(base[2], acc0)
    for m in shifts:
        assert same(call(m), base), m


@pytest.mark.parametrize("last", [False, True])
def test_harmonic_osc_stream(last):
    from golf_amd import functional as GF

    B, Tp, P, A, H = 2, 41, 120, 240, 20
    N = (Tp - 1) * P + 1
    Fa = (N - 1) // A + 1
    rng = np.random.default_rng(41)
    ph = dev((rng.uniform(80, 1000, (B, 1)) * (1 + 0.03 * np.sin(np.linspace(0, 20, Tp))[None]) / 24000).astype(np.float32))
    amp = dev((rng.uniform(0, 1, (B, Fa, H)) / np.arange(1, H + 1)).astype(np.float32))
    ts = torch.rsqrt(0.5 / ph)
    acc0 = torch.tensor(rng.integers(-2 ** 62, 2 ** 62, B)).cuda()
    j, nseg = (28, 12) if last else (10, 12)
    t_lo, t_hi = j * P, (j + nseg) * P - 1 + int(last)
    row = lambda t, hop, end: min(t // hop, end - 2) if last else t // hop
    a_rows = slice(row(t_lo, A, Fa), row(t_hi, A, Fa) + 2)
    s_rows = slice(row(t_lo, P, Tp), row(t_hi, P, Tp) + 2)
    assert j + nseg == (Tp - 1 if last else 22) and a_rows.start > 0 and a_rows.stop <= Fa and s_rows.stop <= Tp

    def call(D):
        assert (D * P) % A == 0   # the amplitude track moves by a whole number of rows
        da, acc = D * P // A, acc0.clone()
        out = GF.harmonic_osc_stream(ph[:, j:j + nseg + 1], j + D, nseg, last, P, H, acc, amp=amp[:, a_rows],
                                     a_first=a_rows.start + da, a_end=Fa + da if last else -1, amp_hop=A, tscale=ts[:, s_rows],
                                     s_first=s_rows.start + D, s_end=Tp + D if last else -1, ts_hop=P)
        return out, acc

    # the entry caps (j0 + nseg + 1) P at 2^40: the far shift ends just under it (and above 2^39: beyond an unsigned cast)
    near = far_shifts(P, 2)[0]
    far = (((1 << 40) // P - Tp - 1) // 2) * 2
    assert (far + j + nseg + 1) * P <= 1 << 40 < (far + Tp + 4) * P
    near_s, far_s = near * P, far * P
    assert 1 << 31 <= near_s + t_lo and near_s + t_hi < WRAP and far_s + t_lo > 1 << 39 and near_s % WRAP and far_s % WRAP
    base = call(0)
    assert base[0].shape == (B, nseg * P + int(last)) and base[0].abs().max() > 0.1 and not torch.equal(base[1], acc0)
    for D in (near, far):
        assert same(call(D), base), D


# ---- the fixed-lag path search ----------------------------------------------------------------------------------------------
def test_f0_viterbi_stream():
    """The entry refuses f_done + nf >= 2^31: one shift, with the last frame just below.  The carry keeps frame f at f % lag
    and the kernel's LDS rings at f % VS_RING (2048), so the shift is a multiple of both."""
    import f0_track_ref as TR
    from golf_amd import functional as GF

    F, K, lag, ring = 130, 7, 12, 2048
    p, a = (dev(t) for t in TR.random_candidates(F, K, 0))
    B = p.shape[0]
    period = lag * ring // math.gcd(lag, ring)
    D = (((1 << 31) - 1 - F) // period) * period
    assert D % lag == 0 and D % ring == 0 and D % WRAP and (1 << 31) - period <= D + F < 1 << 31
    carry0 = GF.f0_viterbi_stream_state(B, K, lag, "cuda")
    cuts = [40, 70, 100, 130]

    def chain(D, carry, lo):
        outs = []
        for f0, f1 in zip([lo] + cuts, cuts):
            if f1 > lo:
                outs += GF.f0_viterbi_stream(p[:, f0:f1], a[:, f0:f1], carry, f0 + D, lag, 24000.0, 24.0, flush=f1 == F,
                                             return_state=True, **TR.COSTS)
                outs.append(carry.clone())
        return outs

    head = chain(0, carry0, 0)[:3]        # frames [0, 40): the carry an ordinary chain from 0 leaves behind
    start = head[2]
    base = chain(0, start.clone(), 40)
    assert len(base) == 9 and sum(t.shape[1] for t in [head[0]] + base[0::3]) == F and (torch.cat(base[1::3], 1) > 0).any()
    whole = GF.f0_viterbi_stream(p, a, GF.f0_viterbi_stream_state(B, K, lag, "cuda"), 0, lag, 24000.0, 24.0, flush=True,
                                 return_state=True, **TR.COSTS)
    assert torch.equal(torch.cat([head[0]] + base[0::3], 1), whole[0]) and torch.equal(torch.cat([head[1]] + base[1::3], 1), whole[1])
    assert same(chain(D, start.clone(), 40), base)
