"""The plain side of the harmonic oscillator bank's tests (csrc/glottal_osc.hip: harm_kernel<DERIV>, harm_bwd_kernel,
harm_bwd_combine_kernel behind functional.harmonic_osc): a float64 closed form of the op and of its five gradients, the host
formulas of the launch (blocks, scan tiles, amplitude segments, staged rows, LDS bytes, what the host check refuses), and the
table of cases with their inputs.  numpy float64, no GPU: tests/test_harm_ref_host.py checks this file,
tests/test_gpu_harmonic_edges.py runs the kernels on its cases.  (``dense_torch`` at the end is not part of the reference: the
reference module's formula restated on torch tensors, for autograd in float64 on the host and in fp32 on the device.)

The op, every operand optional and each at its own hop (up = linear upsampling, (n-1)*hop+1 samples):
    p = up(phase), Phi = cumsum(p), theta_h = h (Phi + up(offset)) + initial_phase[b,h], mask = h p < 0.5
    y = up(tscale) * sum_h mask * up(amp)[.,h] * hscale[h] * sin(2 pi theta_h),   length = the shortest upsampled track

Mask condition, not a tolerance.  The kernel forms p as fmaf(k, (p1-p0)/P, p0) and compares (float)h * p < 0.5f; against exact
arithmetic that is off by less than about 1e-7 in h p near 0.5 (an ulp of 0.5 is 3e-8).  ``inputs`` draws a case from the
seeds case.seed, case.seed+1, .. (at most 32) and takes the first whose ``margin`` = min |h p - 0.5| over all samples and
h <= H is at least MARGIN = 1e-6, ten times that: both sides then evaluate the same mask, no sample is excluded from any
comparison and no bar carries an allowance for a flipped harmonic.  The planted cases are the exception by design: at
phase_hop = 1 p is an input value, and the planted values give products that are 0.5 exactly or within an fp32 ulp of it and
for which the fp32 comparison and the float64 one agree (``planted_masks_agree``).

Drawn inputs: f0 of row b geometric-uniform in the b-th of B equal log-slices of [f0lo, f0hi] Hz at 24 kHz (so a batch
always holds a low and a high voice and the mask cuts at different harmonics in different rows) with 3 % vibrato; amplitudes
U(0,1)/h; tscale U(0.5,1.5); hscale U(0.5,1.5); initial_phase U(-1,1) cycles; phase_offset U(-0.5,0.5) cycles (the kernel
interpolates the offset in fp32 before it takes the fraction: an offset of magnitude x carries x * 6e-8 cycles of rounding,
times 2 pi h in harmonic h's argument, so whole cycles of offset would spend the 2e-5 bar of y on the input's own rounding);
cotangent N(0,1)."""
from collections import namedtuple

import numpy as np

MARGIN = 1e-6
SEEDS = 32
SR = 24000.0
BLOCK = 256                # HARM_THREADS: output samples per block of harm_kernel
SCAN_TILE = 1024           # OSC_SCAN_TILE: phase samples per scan tile
STATIC_LDS = 8 * (256 + 4)   # harm_kernel's toff[256] + twsum[4], 64-bit words
LDS_LIMIT = 64 * 1024
QUANTITIES = ("y", "dphi", "g_phase", "g_amp", "g_tscale", "g_offset", "g_initial_phase")
BARS = dict(y=2e-5, g_amp=2e-5, dphi=1e-4, g_phase=1e-4, g_tscale=1e-4, g_offset=1e-4, g_initial_phase=1e-4)


# ---- the op in float64 ---------------------------------------------------------------------------------------------------
def up_len(n, hop):
    return (n - 1) * hop + 1 if hop > 1 else n


def up(x, hop):
    """Linear upsampling along axis 1 (align_corners): out[f*hop + r] = x[f] (1 - r/hop) + x[f+1] r/hop, (F-1)*hop+1 samples."""
    x = np.asarray(x, dtype=np.float64)
    F = x.shape[1]
    if hop == 1 or F == 1:
        return x.copy()
    n = np.arange((F - 1) * hop + 1)
    f = np.minimum(n // hop, F - 2)
    w = ((n - f * hop) / hop).reshape((1, -1) + (1,) * (x.ndim - 2))
    return x[:, f] * (1.0 - w) + x[:, f + 1] * w


def up_adjoint(v, hop, F):
    """The transpose of ``up`` restricted to its first T = v.shape[1] output samples: (B,T,...) -> (B,F,...)."""
    v = np.asarray(v, dtype=np.float64)
    B, T = v.shape[:2]
    out = np.zeros((B, F) + v.shape[2:])
    if hop == 1 or F == 1:
        out[:, :T] = v
        return out
    n = np.arange(T)
    f = np.minimum(n // hop, F - 2)
    w = ((n - f * hop) / hop).reshape((-1,) + (1,) * (v.ndim - 2))
    for b in range(B):
        np.add.at(out[b], f, v[b] * (1.0 - w))
        np.add.at(out[b], f + 1, v[b] * w)
    return out


def harmonic(phase, phase_hop, H, amp=None, amp_hop=1, tscale=None, ts_hop=1, hscale=None, offset=None, po_hop=1,
             initial_phase=None, gy=None):
    """y and dy/dPhi of the bank in float64 on the given (fp32) inputs, and with a cotangent ``gy`` every gradient that exists
    for the operands given: {"y", "dphi", "p", "mask", "g_phase", "g_amp", "g_tscale", "g_offset", "g_initial_phase"}."""
    phase = np.asarray(phase, dtype=np.float64)
    B, Tp = phase.shape
    p = up(phase, phase_hop)
    T = p.shape[1]
    A = ts = off = None
    if amp is not None:
        A = up(amp, amp_hop)
        T = min(T, A.shape[1])
    if tscale is not None:
        ts = up(tscale, ts_hop)
        T = min(T, ts.shape[1])
    if offset is not None:
        off = up(offset, po_hop)
        T = min(T, off.shape[1])
    h = np.arange(1, H + 1, dtype=np.float64)
    Phi = np.cumsum(p, axis=1)[:, :T]
    p = p[:, :T]
    base = Phi if off is None else Phi + off[:, :T]
    theta = base[:, :, None] * h
    if initial_phase is not None:
        theta = theta + np.asarray(initial_phase, dtype=np.float64)[:, None, :]
    theta = theta - np.floor(theta)
    mask = p[:, :, None] * h < 0.5
    w = mask.astype(np.float64)                      # mask * hscale: what multiplies up(amp) sin
    if hscale is not None:
        w = w * np.asarray(hscale, dtype=np.float64)
    wa = w if A is None else w * A[:, :T]            # mask * hscale * up(amp)
    S, C = np.sin(2 * np.pi * theta), np.cos(2 * np.pi * theta)
    y0 = (wa * S).sum(-1)
    d0 = 2 * np.pi * (wa * h * C).sum(-1)
    tsT = 1.0 if ts is None else ts[:, :T]
    out = dict(y=tsT * y0, dphi=tsT * d0, p=p, mask=mask)
    if gy is None:
        return out
    gy = np.asarray(gy, dtype=np.float64)
    assert gy.shape == (B, T), (gy.shape, B, T)
    g = gy * tsT
    gd = gy * out["dphi"]
    out["g_phase"] = up_adjoint(np.cumsum(gd[:, ::-1], axis=1)[:, ::-1], phase_hop, Tp)
    if amp is not None:
        out["g_amp"] = up_adjoint(g[:, :, None] * w * S, amp_hop, np.asarray(amp).shape[1])
    if tscale is not None:
        out["g_tscale"] = up_adjoint(gy * y0, ts_hop, np.asarray(tscale).shape[1])
    if offset is not None:
        out["g_offset"] = up_adjoint(gd, po_hop, np.asarray(offset).shape[1])
    if initial_phase is not None:
        out["g_initial_phase"] = 2 * np.pi * np.einsum("bt,bth->bh", g, wa * C)
    return out


def margin_of(phase, phase_hop, H, T=None):
    """min |h p - 0.5| over the samples (the first T) and h = 1 .. H, p = up(phase) in float64."""
    p = up(phase, phase_hop)[:, :T].ravel()
    p = p[p > 0]
    if p.size == 0:
        return 0.5
    lo = np.clip(np.floor(0.5 / p), 1, H)
    hi = np.minimum(lo + 1, H)
    return float(min(np.abs(lo * p - 0.5).min(), np.abs(hi * p - 0.5).min()))


# ---- the table -----------------------------------------------------------------------------------------------------------
# Fa / Fs / Fo = 0: no amplitudes / tscale / phase_offset.  blocks, tiles, segs, ends are CLAIMS: what the case was built to
# have; tests/test_harm_ref_host.py holds them against ``geometry``.  ends names the track(s) whose upsampled length is the
# output's.  grads = "all": every gradient the operands have; "long": forward, g_amp, g_phase.
Case = namedtuple("Case", "name B H Tp ph Fa ah Fs sh Fo oh hs ip voice f0 seed blocks tiles segs ends edge grads")


def _case(name, B, H, Tp, ph, amp=(0, 1), ts=(0, 1), off=(0, 1), hs=False, ip=False, voice="voiced", f0=(80, 1000),
          blocks=0, tiles=1, segs=0, ends="phase", edge="", grads="all"):
    return Case(name, B, H, Tp, ph, amp[0], amp[1], ts[0], ts[1], off[0], off[1], hs, ip, voice, f0, 0, blocks, tiles, segs,
                ends, edge, grads)


# planted increments (cycles per sample), each held for PLANT_RUN samples: 2 p = 0.5 exactly; 2 p = 0.5 and 4 p = ..; 4 p = 0.5;
# 3 p = 0.5 + 2^-26 in float64 and 0.5 after fp32 rounding; 2 p one fp32 ulp above / below 0.5
PLANTED = (0.5, 0.25, 0.125, float(np.float32(1.0 / 6.0)), float(np.float32(0.25) * (1 + np.float32(2.0 ** -23))),
           float(np.float32(0.25) * (1 - np.float32(2.0 ** -23))))
PLANT_RUN = 45

_OPS = [_case(f"ops-a{a}s{s}h{hs}o{o}i{i}", 2, 33, 151, 4, amp=(87 * a, 7), ts=(68 * s, 9), off=(122 * o, 5), hs=bool(hs),
              ip=bool(i), blocks=3, segs=86 * a, edge="operand subset")
        for a in (0, 1) for s in (0, 1) for hs in (0, 1) for o in (0, 1) for i in (0, 1)]

_HARMONICS = [_case(f"H{H}", 3, H, 700, 1, amp=(12, 64), ts=(45, 16), off=(23, 32), hs=True, ip=True, blocks=3, segs=11,
                    edge="harmonic count at a 32-anchor boundary")
              for H in (1, 31, 32, 33, 64, 65, 155)]

_ALL = dict(hs=True, ip=True)
_ENDS = [
    _case("ends-phase-by1", 2, 33, 153, 4, (88, 7), (69, 9), (123, 5), blocks=3, segs=87, ends="phase",
          edge="phase shortest by one sample", **_ALL),
    _case("ends-phase-block", 2, 33, 76, 4, (88, 7), (69, 9), (123, 5), blocks=2, segs=87, ends="phase",
          edge="phase shortest by more than a block: trailing amplitude segments hold no sample", **_ALL),
    _case("ends-amp-by1", 2, 33, 150, 4, (86, 7), (68, 9), (121, 5), blocks=3, segs=85, ends="amp",
          edge="amp shortest by one sample", **_ALL),
    _case("ends-amp-block", 2, 33, 151, 4, (44, 7), (68, 9), (122, 5), blocks=2, segs=43, ends="amp",
          edge="amp shortest by more than a block", **_ALL),
    _case("ends-tscale-by1", 2, 33, 152, 4, (88, 7), (68, 9), (122, 5), blocks=3, segs=87, ends="tscale",
          edge="tscale shortest by one sample", **_ALL),
    _case("ends-tscale-block", 2, 33, 151, 4, (87, 7), (34, 9), (122, 5), blocks=2, segs=86, ends="tscale",
          edge="tscale shortest by more than a block", **_ALL),
    _case("ends-offset-by1", 2, 33, 150, 4, (87, 7), (68, 9), (120, 5), blocks=3, segs=86, ends="offset",
          edge="offset shortest by one sample", **_ALL),
    _case("ends-offset-block", 2, 33, 151, 4, (87, 7), (68, 9), (61, 5), blocks=2, segs=86, ends="offset",
          edge="offset shortest by more than a block", **_ALL),
    _case("ends-offset-noamp-ip", 2, 33, 151, 4, off=(61, 5), blocks=2, ends="offset",
          edge="offset ends the output of the initial_phase pseudo-frame path", **_ALL),
]


def _cover(T, hop):
    return T if hop == 1 else -(-(T - 1) // hop) + 1


# output lengths around the block size; initial_phase without amplitudes: the wrapper's pseudo-frames switch at 257 / 258
_TOUT = [_case(f"Tout{T}", 2, 7, T, 1, ts=(_cover(T, 5), 5), off=(_cover(T, 3), 3), blocks=-(-T // 256), ends=e,
               edge="output length at a block edge; pseudo-frame switch" + ("; Fs = Fo = 1" if T == 1 else ""), **_ALL)
         for T, e in ((1, "phase+tscale+offset"), (2, "phase"), (255, "phase"), (256, "phase+tscale+offset"), (257, "phase"),
                      (258, "phase"), (512, "phase"), (513, "phase"))]

_AMP_HOP = [
    _case("amp-hop1", 2, 33, 700, 1, (700, 1), ip=True, blocks=3, segs=699, ends="phase+amp", edge="amp_hop 1"),
    _case("amp-hop3", 2, 33, 700, 1, (234, 3), ip=True, blocks=3, segs=233, ends="phase+amp", edge="amp_hop 3: off the block"),
    _case("amp-hop7", 2, 33, 700, 1, (101, 7), ip=True, blocks=3, segs=100, edge="amp_hop 7: off the block"),
    _case("amp-hop100", 2, 33, 700, 1, (8, 100), ip=True, blocks=3, segs=7, edge="amp_hop 100: fewer than nrows rows left"),
    _case("amp-hop255", 2, 33, 700, 1, (4, 255), ip=True, blocks=3, segs=3, edge="amp_hop 255"),
    _case("amp-hop256-clamped", 2, 33, 700, 1, (3, 256), ip=True, blocks=3, segs=2, ends="amp",
          edge="amp_hop 256; the last block's row_lo clamped to Fa - 2"),
    _case("amp-hop257", 2, 33, 700, 1, (4, 257), ip=True, blocks=3, segs=3, edge="amp_hop 257: above the block"),
    _case("amp-hop300", 2, 33, 700, 1, (4, 300), ip=True, blocks=3, segs=3, edge="amp_hop 300: above the block"),
    _case("amp-hop-beyond", 2, 33, 700, 1, (2, 1000), ip=True, blocks=3, segs=1, edge="amp_hop beyond the output: one segment"),
    _case("amp-Fa1", 2, 33, 5, 1, (1, 64), ip=True, blocks=1, segs=1, ends="amp", edge="Fa = 1: one-sample output"),
    _case("amp-hop1-H59", 1, 59, 300, 1, (300, 1), ip=True, f0=(80, 400), blocks=2, segs=299, ends="phase+amp",
          edge="amp_hop 1 at the largest H the host check admits"),
]

_TRACK_HOP = [_case(f"track-hop{k}", 2, 9, 700, 1, (12, 64), (_cover(700, k), k), (_cover(700, k), k), blocks=3, segs=11,
                    ends="phase" if (699 % k) else "phase+tscale+offset", edge=f"ts_hop = po_hop = {k}")
              for k in (1, 3, 7, 100, 255, 256, 257, 300)]
_TRACK_HOP.append(_case("track-hop-beyond", 2, 9, 700, 1, (12, 64), (2, 1000), (2, 1000), blocks=3, segs=11,
                        edge="ts_hop = po_hop beyond the output"))

_PHASE = [
    _case("ph1-Tp1", 2, 9, 1, 1, (2, 60), (2, 40), ip=True, blocks=1, segs=1, edge="Tp 1"),
    _case("ph1-Tp2", 2, 9, 2, 1, (2, 60), (2, 40), ip=True, blocks=1, segs=1, edge="Tp 2"),
    _case("ph1-Tp1024", 2, 9, 1024, 1, (19, 60), (27, 40), ip=True, blocks=4, segs=18, edge="Tp 1024: one full scan tile"),
    _case("ph1-Tp1025", 2, 9, 1025, 1, (19, 60), (27, 40), ip=True, blocks=5, tiles=2, segs=18, edge="Tp 1025: second tile"),
    _case("ph1-Tp2049", 2, 9, 2049, 1, (36, 60), (53, 40), ip=True, blocks=9, tiles=3, segs=35, edge="Tp 2049: third tile"),
    _case("ph2-Tp1025", 2, 9, 1025, 2, (36, 60), (53, 40), ip=True, blocks=9, tiles=2, segs=35, edge="phase_hop 2"),
    _case("ph37-Tp2", 2, 9, 2, 37, (2, 60), (2, 40), ip=True, blocks=1, segs=1, edge="phase_hop 37, one segment"),
    _case("ph37-Tp30", 2, 9, 30, 37, (19, 60), (28, 40), ip=True, blocks=5, segs=18, edge="phase_hop 37"),
    _case("ph120-Tp1", 2, 9, 1, 120, (2, 60), (2, 40), ip=True, blocks=1, segs=1, edge="phase_hop 120, a lone frame"),
    _case("ph120-Tp9", 2, 9, 9, 120, (17, 60), (25, 40), ip=True, blocks=4, segs=16, ends="phase+amp+tscale",
          edge="phase_hop 120"),
    _case("long-66tiles", 2, 3, 66561, 1, (279, 240), blocks=261, tiles=66, segs=278, grads="long",
          edge="66 scan tiles: the prefix across waves"),
    _case("long-256tiles", 2, 3, 262144, 1, (1094, 240), blocks=1024, tiles=256, segs=1093, grads="long",
          edge="256 scan tiles: the last LDS-prefix size"),
    _case("long-257tiles", 2, 3, 262145, 1, (1094, 240), blocks=1025, tiles=257, segs=1093, grads="long",
          edge="257 scan tiles: the folded long path"),
]

_MASK = [
    _case("planted", 2, 8, len(PLANTED) * PLANT_RUN, 1, (18, 16), (10, 30), hs=True, ip=True, voice="planted", blocks=2,
          segs=17, ends="phase", edge="h p exactly 0.5 or one fp32 ulp either side"),
    _case("unvoiced-ph16", 2, 33, 40, 16, (27, 24), (14, 50), hs=True, ip=True, voice="unvoiced", f0=(300, 2000), blocks=3,
          segs=26, ends="phase+amp", edge="p == 0 stretches and ramps in and out of them"),
    _case("unvoiced-ph1", 2, 33, 625, 1, (27, 24), (14, 50), hs=True, ip=True, voice="unvoiced", f0=(300, 2000), blocks=3,
          segs=26, ends="phase+amp", edge="p == 0 stretches and ramps, p an input value"),
]

_LDS = [
    _case("lds-max-noamp", 2, 3965, 300, 1, ts=(11, 30), hs=True, ip=True, f0=(2, 40), blocks=2, ends="phase",
          edge="the largest H with initial_phase and no amplitudes: 65 532 bytes"),
    _case("lds-max-amp256", 1, 2266, 400, 1, (3, 256), hs=True, ip=True, f0=(3, 60), blocks=2, segs=2, ends="phase",
          edge="the largest H with initial_phase at amp_hop 256: 65 536 bytes"),
]

CASES = _OPS + _HARMONICS + _ENDS + _TOUT + _AMP_HOP + _TRACK_HOP + _PHASE + _MASK + _LDS
CASES = [c._replace(seed=1000 * i) for i, c in enumerate(CASES)]
assert len({c.name for c in CASES}) == len(CASES)


# mask-safe tracks for the modules (AudioTensor hops must divide each other): phase at the sample rate and at hop 4
MODULE_CASES = [
    _case("module-ph1", 2, 20, 600, 1, (6, 120), f0=(200, 2000), blocks=3, segs=5, edge="modules, phase at hop 1")._replace(seed=900000),
    _case("module-ph4", 2, 20, 150, 4, (76, 8), blocks=3, segs=75, edge="modules, phase at hop 4")._replace(seed=901000),
]


def case_id(c):
    return c.name


def case(name):
    return next(c for c in CASES + MODULE_CASES if c.name == name)


# ---- the host formulas of the launch -------------------------------------------------------------------------------------
def lengths(c):
    """{track: upsampled length} of the tracks a case has."""
    out = {"phase": up_len(c.Tp, c.ph)}
    if c.Fa:
        out["amp"] = up_len(c.Fa, c.ah)
    if c.Fs:
        out["tscale"] = up_len(c.Fs, c.sh)
    if c.Fo:
        out["offset"] = up_len(c.Fo, c.oh)
    return out


def nrows_of(amp_hop):
    return BLOCK // amp_hop + 3


def lds_bytes_of(H, Fa, amp_hop, ip):
    """What a harm_kernel launch asks for: static arrays + hs (padded to 4) + the staged rows + cos / sin of initial_phase."""
    return STATIC_LDS + 4 * (((H + 3) & ~3) + (nrows_of(amp_hop) if Fa else 1) * H + (2 * H if ip else 0))


def refusal_of(H, Fa, amp_hop, ip):
    """None, or why the host check refuses the forward launch (GOLF_EUNSUPPORTED)."""
    if Fa and (nrows_of(amp_hop) + 1) * H * 4 > 60 * 1024:
        return "rows"
    if lds_bytes_of(H, Fa, amp_hop, ip) > LDS_LIMIT:
        return "lds"
    return None


Geometry = namedtuple("Geometry", "Tout blocks tiles segs nrows lds ends pseudo")


def geometry(c):
    L = lengths(c)
    Tout = min(L.values())
    pseudo = None
    if c.ip and not c.Fa:      # d / d initial_phase without amplitudes: (frames, hop) of the wrapper's pseudo-frames
        hq = 256 if Tout > 257 else max(Tout - 1, 1)
        pseudo = (-(-(Tout - 1) // hq) + 1 if Tout > 1 else 2, hq)
    return Geometry(Tout, -(-Tout // BLOCK), -(-c.Tp // SCAN_TILE), max(c.Fa - 1, 1) if c.Fa else 0, nrows_of(c.ah) if c.Fa else 0,
                    lds_bytes_of(c.H, c.Fa, c.ah, c.ip), "+".join(k for k, v in L.items() if v == Tout), pseudo)


def staged_rows(c):
    """Per block of a case with amplitudes: (t_lo // amp_hop, row_lo, rows staged), as harm_kernel computes them."""
    g = geometry(c)
    out = []
    for blk in range(g.blocks):
        q = blk * BLOCK // c.ah
        row_lo = min(q, c.Fa - 2) if c.Fa >= 2 else 0
        out.append((q, row_lo, min(g.nrows, c.Fa - row_lo)))
    return out


def empty_amp_rows(c):
    """Amplitude rows no output sample touches (their g_amp is exactly zero): row f has weight on samples in ((f-1) hop, (f+1) hop)."""
    Tout = geometry(c).Tout
    return [f for f in range(c.Fa) if (f - 1) * c.ah + 1 > Tout - 1] if c.ah > 1 else list(range(Tout, c.Fa))


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _phase_track(c, rng):
    if c.voice == "planted":
        rows = [np.repeat(np.roll(PLANTED, -b), PLANT_RUN) for b in range(c.B)]
        return np.asarray(rows, dtype=np.float32)
    lo, hi = c.f0
    b = np.arange(c.B)[:, None]
    f0 = lo * (hi / lo) ** ((b + rng.uniform(0, 1, (c.B, 1))) / c.B)
    vib = 1 + 0.03 * np.sin(np.linspace(0, 20, c.Tp)[None] + rng.uniform(0, 6, (c.B, 1)))
    p = f0 * vib / SR
    if c.voice == "unvoiced":   # frames: voiced | ramp | zeros | ramp | voiced | zeros to the end (at hop 1: linear ramps drawn)
        n = c.Tp
        gate = np.ones(n)
        a, z, r = n // 5, n // 8, max(n // 10, 1) if c.ph == 1 else 1
        gate[a:a + r] = np.linspace(1, 0, r + 2)[1:-1] if c.ph == 1 else 0.0
        gate[a + r:a + r + z] = 0.0
        gate[a + r + z:a + 2 * r + z] = np.linspace(0, 1, r + 2)[1:-1] if c.ph == 1 else 1.0
        gate[n - z:] = 0.0
        if c.ph == 1:
            gate[n - z - r:n - z] = np.linspace(1, 0, r + 2)[1:-1]
        p = p * gate[None]
    return p.astype(np.float32)


def _draw(c, seed):
    rng = np.random.default_rng(seed)
    h = np.arange(1, c.H + 1)
    d = dict(phase=_phase_track(c, rng), amp=None, tscale=None, hscale=None, offset=None, initial_phase=None)
    if c.Fa:
        d["amp"] = (rng.uniform(0, 1, (c.B, c.Fa, c.H)) / h).astype(np.float32)
    if c.Fs:
        d["tscale"] = rng.uniform(0.5, 1.5, (c.B, c.Fs)).astype(np.float32)
    if c.hs:
        d["hscale"] = rng.uniform(0.5, 1.5, c.H).astype(np.float32)
    if c.Fo:
        d["offset"] = rng.uniform(-0.5, 0.5, (c.B, c.Fo)).astype(np.float32)
    if c.ip:
        d["initial_phase"] = rng.uniform(-1, 1, (c.B, c.H)).astype(np.float32)
    d["gy"] = rng.normal(0, 1, (c.B, geometry(c).Tout)).astype(np.float32)
    return d


_inputs, _refs = {}, {}


def inputs(c):
    """The case's fp32 arrays (read-only, made once): phase, amp, tscale, hscale, offset, initial_phase (None where absent),
    gy, and "seed" / "margin" of the draw.  The first of SEEDS seeds whose margin holds; the planted case keeps its own."""
    if c.name in _inputs:
        return _inputs[c.name]
    Tout = geometry(c).Tout
    for seed in range(c.seed, c.seed + SEEDS):
        d = _draw(c, seed)
        m = margin_of(d["phase"], c.ph, c.H, Tout)
        if m >= MARGIN or c.voice == "planted":
            d.update(seed=seed, margin=m)
            _inputs[c.name] = _frozen(d)
            return d
    raise AssertionError(f"{c.name}: no seed in {c.seed} .. {c.seed + SEEDS - 1} keeps h p {MARGIN} away from 0.5")


def margin(c):
    return inputs(c)["margin"]


def operands(c, d=None):
    """The keyword arguments of ``harmonic`` (and, with tensors for arrays, of functional.harmonic_osc) for a case."""
    d = inputs(c) if d is None else d
    return dict(phase_hop=c.ph, amp=d["amp"], amp_hop=c.ah, tscale=d["tscale"], ts_hop=c.sh, hscale=d["hscale"],
                offset=d["offset"], po_hop=c.oh, initial_phase=d["initial_phase"])


def wanted(c):
    """The quantities a case is compared on."""
    q = ["y", "dphi", "g_phase"] + ["g_" + k for k, on in (("amp", c.Fa), ("tscale", c.Fs), ("offset", c.Fo),
                                                             ("initial_phase", c.ip)) if on]
    return [k for k in q if c.grads == "all" or k in ("y", "g_amp", "g_phase")]


def refs(c):
    """The float64 reference of a case (read-only, computed once)."""
    if c.name not in _refs:
        d = inputs(c)
        _refs[c.name] = _frozen(harmonic(d["phase"], H=c.H, gy=d["gy"], **operands(c, d)))
    return _refs[c.name]


def planted_masks_agree(phase, H):
    """For increments that are input values (phase_hop 1): the comparison the kernel makes, (float)h * p < 0.5f in fp32, and
    the float64 one give the same mask for every sample and h <= H.  Returns (agree, number of (sample, h) within an fp32
    ulp of 0.5)."""
    p32 = np.asarray(phase, dtype=np.float32)
    h32 = np.arange(1, H + 1, dtype=np.float32)
    m32 = (p32[..., None] * h32).astype(np.float32) < np.float32(0.5)
    prod = p32.astype(np.float64)[..., None] * h32.astype(np.float64)
    return bool((m32 == (prod < 0.5)).all()), int((np.abs(prod - 0.5) <= 2.0 ** -24).sum())


def distances(got, want):
    """(rel-max, rel-l2) as conftest.rel_err measures them."""
    from conftest import rel_err

    return rel_err(got, want)


# ---- the dense formula in torch --------------------------------------------------------------------------------------------
def dense_torch(phase, H, phase_hop=1, amp=None, amp_hop=1, tscale=None, ts_hop=1, hscale=None, offset=None, po_hop=1,
                initial_phase=None, eps=None):
    """models/synth.py:403-446 restated densely on torch tensors of any dtype / device (interpolate, cumsum, mask, sin), with
    the per-sample and per-harmonic scales as the subclasses multiply them into the amplitudes.  ``eps`` (B, T) is added to
    the running phase Phi: the gradient of y.sum() w.r.t. a zero eps is dy/dPhi per sample."""
    import torch
    import torch.nn.functional as F

    def upt(x, hop):   # (B, F) or (B, F, H) along dim 1
        if hop == 1 or x.shape[1] == 1:
            return x
        n = (x.shape[1] - 1) * hop + 1
        if x.dim() == 2:
            return F.interpolate(x[:, None], size=n, mode="linear", align_corners=True)[:, 0]
        return F.interpolate(x.transpose(1, 2), size=n, mode="linear", align_corners=True).transpose(1, 2)

    h = torch.arange(1, H + 1, device=phase.device, dtype=phase.dtype)
    p = upt(phase, phase_hop)
    tracks = [t for t in (upt(amp, amp_hop) if amp is not None else None, upt(tscale, ts_hop) if tscale is not None else None,
                          upt(offset, po_hop) if offset is not None else None)]
    T = min([p.shape[1]] + [t.shape[1] for t in tracks if t is not None])
    harmonics = p[:, :, None] * h
    ph = torch.cumsum(harmonics, 1)[:, :T]
    harmonics = harmonics[:, :T]
    if eps is not None:
        ph = ph + eps[:, :, None] * h
    if tracks[2] is not None:
        ph = ph + tracks[2][:, :T, None] * h
    if initial_phase is not None:
        ph = ph + initial_phase[:, None, :]
    A = tracks[0][:, :T] if tracks[0] is not None else torch.ones_like(harmonics)
    if hscale is not None:
        A = A * hscale
    if tracks[1] is not None:
        A = A * tracks[1][:, :T, None]
    A = torch.where(harmonics >= 0.5, torch.zeros_like(A), A)
    return (torch.sin(ph * 2 * torch.pi) * A).sum(-1)
