"""Float64 restatement of the glottal-source match (golf_glottal_match_f32, include/golf_amd.h), written from the definition
with numpy, one step after the other.  It is the checker of csrc/glottal_match.hip (tests/test_gpu_glottal.py) and is itself
pinned on band-limited pulses with a planted table position by tests/test_glottal_host.py.

``fp32=True`` is the stand-in for the kernel's arithmetic: the search with c_h, S and the exponentials rounded to float32,
D = c_h conj(S), the product D E (numpy's float32 matrix product) and rho = C / sqrt(N E2) in float32, the argument h j mod
n_phi still exact; then, as in the kernel, the winner taken again in float64 among the 3 x 3 cells around the float32 one,
the two refinements in float64 and the three outputs rounded to float32.  The GPU test's bars are four times its largest
errors against the float64 version on the GPU test's own cases (profiles/glottal_parity.txt).

Also here: the plan in numpy, the pulse generator and the cases both test files share."""
import numpy as np

import hna_ref

SR, HOP = 24000.0, 240
# what tests/test_glottal_host.py measures on the planted case (profiles/glottal_parity.txt): the float64 restatement's largest
# and rms error of w in table steps and of theta in cycles on interior frames, and the bar between the rho of white noise
# (at most 0.33) and of voiced frames (at least 0.999)
PLANTED_W_MAX, PLANTED_W_RMS, PLANTED_THETA, RHO_BAR = 1.1225, 0.6582, 1.389e-3, 0.66
# and on the same planted tracks rendered as the oscillator renders them (``round_trip_case``): the frames' blended tables
# interpolated over time, four times oversampled and decimated -- the reference of the GPU round trip
ROUND_TRIP_W_MAX = 1.4311
TIE = 1e-5   # a second (k, j), more than one row from the argmax, this close to the largest rho: the frame's w is not compared


def plan(table, H):
    """(S fp32 (K, H, 2), N fp32 (K, H), X fp32 (K - 1, H)) of a table (K, L): S = 2 rfft / L on bins 1..H, zero above L/2;
    the prefix sums of the stored S in float64, rounded once."""
    table = np.asarray(table, np.float64)
    K, L = table.shape
    spec = np.fft.rfft(table, axis=1)[:, 1:H + 1] * (2.0 / L)
    S = np.zeros((K, H, 2), np.float32)
    S[:, :spec.shape[1], 0], S[:, :spec.shape[1], 1] = spec.real, spec.imag
    Sd = S.astype(np.float64)
    N = np.cumsum((Sd * Sd).sum(-1), axis=1).astype(np.float32)
    X = np.cumsum((Sd[:-1] * Sd[1:]).sum(-1), axis=1).astype(np.float32)
    return S, N, X


def live_harmonics(f0v, H, sample_rate):
    """Hf: the harmonics h = 1..H with h (double)f0 / sr < 0.5, the rule of the harmonic analysis; 0 for an unvoiced frame."""
    if not f0v > 0:
        return 0
    omega = float(np.float32(f0v)) / sample_rate
    return int(np.sum(np.arange(1, H + 1) * omega < 0.5))


def refine(c_row, c_prev, c_next, js, ks, N, X, Hf, E2, K, n_phi):
    """Steps 5 and 6 on the scores of row k* (all columns) and of its neighbours at column j* (None where there is none)."""
    ym, y0, yp = float(c_row[(js - 1) % n_phi]), float(c_row[js]), float(c_row[(js + 1) % n_phi])
    curv = ym - 2 * y0 + yp
    d = 0.5 * (ym - yp) / curv if curv != 0 else 0.0
    d = min(max(d, -0.5), 0.5)
    theta = (js + d) / n_phi
    theta -= np.floor(theta)
    nss = float(N[ks, Hf - 1])
    best, wk = (y0 / np.sqrt(nss * E2) if nss > 0 else 0.0), float(ks)
    for ka, c0, c1 in ((ks - 1, c_prev, y0), (ks, y0, c_next)):
        if ka < 0 or ka + 1 >= K:
            continue
        c0, c1 = float(c0), float(c1)
        n00, n11, n01 = float(N[ka, Hf - 1]), float(N[ka + 1, Hf - 1]), float(X[ka, Hf - 1])
        u, v = c1 * n00 - c0 * n01, c0 * n11 - c1 * n01
        p = u / (u + v) if u + v != 0 else 0.0
        p = min(max(p, 0.0), 1.0)
        nb = (1 - p) ** 2 * n00 + 2 * p * (1 - p) * n01 + p * p * n11
        sc = ((1 - p) * c0 + p * c1) / np.sqrt(nb * E2) if nb > 0 else 0.0
        if sc > best:
            best, wk = sc, ka + p
    return wk / (K - 1), theta, best


def match(amp, phase, f0, S, N, X, sample_rate, n_phi, fp32=False):
    """amp, phase (B, F, H) and f0 (B, F) as fp32 values, the plan -> dict: w (NaN where there is no estimate), theta, rho
    (B, F) in float64, and per frame Hf, the argmax k, j, and ``tied``: a second (k, j) more than one row from the argmax lies
    within TIE of the largest rho."""
    amp, phase, f0 = np.asarray(amp, np.float32), np.asarray(phase, np.float32), np.asarray(f0, np.float32)
    S, N, X = np.asarray(S, np.float32), np.asarray(N, np.float32), np.asarray(X, np.float32)
    (B, F, H), K = amp.shape, S.shape[0]
    assert S.shape == (K, H, 2) and N.shape == (K, H) and X.shape == (K - 1, H) and n_phi & (n_phi - 1) == 0
    Sc = S[..., 0].astype(np.float64) + 1j * S[..., 1].astype(np.float64)
    w, theta, rho = np.full((B, F), np.nan), np.zeros((B, F)), np.zeros((B, F))
    Hfs, ks_, js_ = np.zeros((B, F), int), np.zeros((B, F), int), np.zeros((B, F), int)
    tied = np.zeros((B, F), bool)
    jj = np.arange(n_phi)
    for b in range(B):
        for f in range(F):
            Hf = Hfs[b, f] = live_harmonics(f0[b, f], H, sample_rate)
            a = amp[b, f, :Hf].astype(np.float64)
            E2 = float((a * a).sum())
            if Hf == 0 or not E2 > 0:
                continue
            c = a * np.exp(2j * np.pi * (phase[b, f, :Hf].astype(np.float64) - 0.25))
            hj = np.outer(np.arange(1, Hf + 1), jj) % n_phi
            E = np.exp(-2j * np.pi * hj / n_phi)
            nk = N[:, Hf - 1].astype(np.float64)
            C = ((c[None] * Sc[:, :Hf].conj()) @ E).real
            r = np.where(nk[:, None] > 0, C / np.sqrt(np.where(nk > 0, nk, 1.0) * E2)[:, None], 0.0)
            if fp32:
                c32, S32, E32 = c.astype(np.complex64), Sc[:, :Hf].astype(np.complex64), E.astype(np.complex64)
                D = c32[None] * S32.conj()
                C32 = (D.real @ E32.real - D.imag @ E32.imag).astype(np.float32)
                inv = np.where(nk > 0, 1 / np.sqrt(np.where(nk > 0, nk, 1.0) * E2), 0.0).astype(np.float32)
                k32, j32 = divmod(int(np.argmax(C32 * inv[:, None])), n_phi)
                # the winner again, in float64, among the 3 x 3 cells around the float32 one
                cand = sorted((k, (j32 + dj) % n_phi) for k in range(max(k32 - 1, 0), min(k32 + 2, K)) for dj in (-1, 0, 1))
                ks, js = max(cand, key=lambda kj: (r[kj], -kj[0], -kj[1]))
            else:
                ks, js = divmod(int(np.argmax(r)), n_phi)   # the first of equal maxima: the smaller k, then the smaller j
            ks_[b, f], js_[b, f] = ks, js
            far = np.abs(np.arange(K) - ks) > 1
            tied[b, f] = bool(far.any() and r[far].max() >= r[ks, js] - TIE)
            w[b, f], theta[b, f], rho[b, f] = refine(C[ks], C[ks - 1, js] if ks > 0 else None,
                                                     C[ks + 1, js] if ks + 1 < K else None, js, ks, N, X, Hf, E2, K, n_phi)
    if fp32:   # the outputs are stored in float32
        w, theta, rho = (a.astype(np.float32).astype(np.float64) for a in (w, theta, rho))
        theta = np.where(theta >= 1, 0.0, theta)
    return dict(w=w, theta=theta, rho=rho, Hf=Hfs, k=ks_, j=js_, tied=tied)


def errors(out, ref, K):
    """Largest errors of ``out`` against ``ref``: rho, theta (cycles, modulo 1) over the frames with an estimate, w in table
    steps over those that are not ``tied`` in ``ref``; and the fraction of voiced frames left out of the w comparison.  The
    frames without an estimate must be the same, NaN / 0 / 0 in both."""
    none = np.isnan(ref["w"])
    assert (np.isnan(out["w"]) == none).all() and (out["theta"][none] == 0).all() and (out["rho"][none] == 0).all()
    ok = ~none
    e_rho = np.abs(out["rho"] - ref["rho"])[ok].max(initial=0.0)
    dt = np.abs(out["theta"] - ref["theta"])
    e_theta = np.minimum(dt, 1 - dt)[ok].max(initial=0.0)
    cmp = ok & ~ref["tied"]
    e_w = (np.abs(out["w"] - ref["w"])[cmp] * (K - 1)).max(initial=0.0)
    return e_rho, e_theta, e_w, float((ok & ref["tied"]).sum()) / max(int(ok.sum()), 1)


# ---- signals -------------------------------------------------------------------------------------------------------------
def spectrum(table, H):
    """The complex S (K, H) of ``plan`` in float64, not rounded."""
    table = np.asarray(table, np.float64)
    spec = np.fft.rfft(table, axis=1)[:, 1:H + 1] * (2.0 / table.shape[1])
    out = np.zeros((table.shape[0], H), complex)
    out[:, :spec.shape[1]] = spec
    return out


def pulses(f0, w, Sc, hop, sample_rate, phi0=0.0):
    """Band-limited pulses of a table in float64: f0 (F) in Hz and w (F) in [0, 1] are upsampled linearly, the table phase
    is Phi[t] = phi0 + sum_{0<s<=t} f0[s] / sr, the spectrum at t the blend of the rows k0 = floor(w (K-1)) and k0 + 1 that
    the oscillator takes, harmonics at or above Nyquist muted.  -> (x ((F-1) hop + 1), Phi)."""
    p = hna_ref.upsample(np.asarray(f0, np.float64), hop) / sample_rate
    wu = hna_ref.upsample(np.asarray(w, np.float64), hop) * (Sc.shape[0] - 1)
    Phi = phi0 + np.cumsum(p) - p[0]
    k0 = np.clip(np.floor(wu).astype(int), 0, Sc.shape[0] - 2)
    q = (wu - k0)[:, None]
    Sb = Sc[k0] * (1 - q) + Sc[k0 + 1] * q
    h = np.arange(1, Sc.shape[1] + 1)
    x = ((Sb * np.exp(2j * np.pi * np.outer(Phi, h))).real * (np.outer(p, h) < 0.5)).sum(1)
    return x, Phi


def random_walk(F, rng, step=0.02, lo=0.1, hi=0.9):
    w = np.clip(rng.uniform(lo, hi) + np.cumsum(rng.normal(0, step, F)), lo, hi)
    return w


_cache = {}


def golf_table():
    """The package's own 100 x 1000 table (float32)."""
    if "table" not in _cache:
        from golf_amd.synth import GlottalFlowTable

        _cache["table"] = GlottalFlowTable().table.detach().numpy().astype(np.float32)
    return _cache["table"]


def glide(F, hop=HOP, sample_rate=SR):
    t = np.arange(F) * hop / sample_rate
    return np.linspace(110.0, 180.0, F) * 2 ** (0.3 / 12 * np.sin(2 * np.pi * 5.5 * t))


def build_case(table, H, n_phi, tracks, ws, seed, hop=HOP, noise=0.01, phi0=None, f0_given=None, silence=None):
    """Pulses of ``table`` on the f0 tracks (Hz per frame) and w tracks, one row each, with white noise at ``noise`` times
    the row's rms -> dict(x fp32 (B, T), f0 fp32 (B, F) as handed to the analysis (``f0_given`` if set), table fp32 (K, L),
    H, n_phi, sample_rate, hop, and what was planted: w (B, F), theta (B, F), the table phase at the frames' centres)."""
    rng = np.random.default_rng(seed)
    Sc = spectrum(table, H)
    xs, th = [], []
    for n, (tr, w) in enumerate(zip(tracks, ws)):
        x, Phi = pulses(tr, w, Sc, hop, SR, 0.0 if phi0 is None else phi0[n])
        x = x + noise * np.sqrt(np.mean(x * x)) * rng.normal(0, 1, len(x))
        if silence is not None:
            x[silence[0]:silence[1]] = 0.0
        xs.append(x)
        th.append(np.mod(Phi[::hop], 1.0))
    f0 = np.array(tracks if f0_given is None else f0_given, np.float32)
    return dict(x=np.array(xs).astype(np.float32), f0=f0, table=np.asarray(table, np.float32), H=H, n_phi=n_phi,
                sample_rate=SR, hop=hop, w=np.array(ws), theta=np.array(th))


PLANTED_F = 40


def planted_tracks():
    """The planted case of the host test and of the GPU round trip: one row, 40 frames, the glide with vibrato and a
    random-walk w -> (f0 (1, F) float64, w (1, F) float64)."""
    return glide(PLANTED_F)[None], random_walk(PLANTED_F, np.random.default_rng(21))[None]


def planted_case(kind="walk", noise=0.01, H=64, n_phi=256):
    """The planted case as pulses of the package's table: ``walk`` (the random-walk w) or ``const`` (w = 0.3)."""
    key = ("planted", kind, noise, H, n_phi)
    if key not in _cache:
        f0, w = planted_tracks()
        if kind == "const":
            w = np.full_like(w, 0.3)
        _cache[key] = build_case(golf_table(), H, n_phi, list(f0), list(w), 22, noise=noise)
    return _cache[key]


def round_trip_case():
    """The planted tracks through the float64 oracle of IndexedGlottalFlowTable(oversampling=4) (oracle/golf_oracle.py): the
    excitation the GPU round trip plants, which ``residual`` returns when the inverse filter undoes the end filter."""
    if "round_trip" not in _cache:
        from oracle import golf_oracle as O

        f0, w = planted_tracks()
        out = O.indexed_glottal_forward((f0 / SR).astype(np.float32), HOP, w.astype(np.float32), HOP,
                                        golf_table().astype(np.float64), oversampling=4,
                                        decim_taps=O.default_decimation_taps(4))["out"]
        _cache["round_trip"] = dict(planted_case(), x=out.astype(np.float32), f0=f0.astype(np.float32))
    return _cache["round_trip"]


def interior(a, edge=2):
    """The frames whose windows lie inside the signal: all but ``edge`` at either end."""
    return a[:, edge:-edge]


def planted_errors(case, out):
    """(largest, rms) error of w in table steps and the largest error of theta in cycles on the interior frames."""
    K = case["table"].shape[0]
    dw = interior(np.abs(out["w"] - case["w"])) * (K - 1)
    dt = np.abs(out["theta"] - case["theta"])
    return float(dw.max()), float(np.sqrt((dw ** 2).mean())), float(interior(np.minimum(dt, 1 - dt)).max())


def cases():
    """name -> a ``build_case`` dict: the inputs of the GPU test, the smallest that reach each edge (B <= 3, F <= 40,
    T <= 9600), which the host test runs through the restatement and its fp32 stand-in."""
    if "cases" in _cache:
        return _cache["cases"]
    c = {}

    def make(name, *args, **kw):
        c[name] = build_case(*args, **kw)

    rng = np.random.default_rng(7)
    # the recipe's sizes: the package's table, a glide with vibrato, a random-walk w; two unvoiced frames and a NaN f0
    F = 40
    tr = [glide(F), glide(F)[::-1].copy()]
    given = np.array(tr, np.float32)
    given[0, [11, 12]] = 0
    given[1, 20] = np.nan
    make("recipe", golf_table(), 64, 256, tr, [random_walk(F, rng), random_walk(F, rng)], 1, f0_given=given)
    # the smallest of everything
    make("smallest", rng.normal(0, 1, (2, 16)), 1, 8, [np.full(9, 150.0)], [np.linspace(0.2, 0.8, 9)], 2)
    # n_phi far above 2 H
    make("n_phi1024", rng.normal(0, 1, (3, 32)), 5, 1024, [np.linspace(200.0, 260.0, 9)], [np.linspace(0.1, 0.9, 9)], 3)
    # H = 256 at 400 Hz: 29 live harmonics, the muted tail, the prefix sums read at column 28
    make("H256_f400", rng.normal(0, 1, (5, 128)), 256, 64, [np.full(9, 400.0)], [np.linspace(0.15, 0.85, 9)], 4)
    # frames at and above Nyquist have no harmonic; the signal is made at 300 Hz
    given = np.full((1, 9), 300.0, np.float32)
    given[0, [2, 3, 6]] = [12000.0, 13000.0, 11999.0]   # 11999 Hz: one harmonic is left
    make("nyquist", rng.normal(0, 1, (4, 64)), 8, 32, [np.full(9, 300.0)], [np.full(9, 0.4)], 5, f0_given=given)
    # frames whose window holds zeros only (a window is at most 480 samples here)
    make("zero_frame", rng.normal(0, 1, (4, 64)), 8, 32, [np.full(11, 200.0)], [np.full(11, 0.6)], 6, silence=(700, 1700))
    # the best row is row 0, row K - 1: one pair to refine with
    make("edge_rows", golf_table()[::11], 32, 128, [np.full(9, 140.0), np.full(9, 210.0)], [np.zeros(9), np.ones(9)], 8)
    # a period of 160 samples and a hop of 160: every frame has the phase the row starts with; j* = 0 and j* = n_phi - 1
    make("wrap", golf_table()[::11], 32, 64, [np.full(9, 150.0), np.full(9, 150.0), np.full(9, 150.0)],
         [np.full(9, 0.35)] * 3, 9, hop=160, phi0=[0.0, 1 - 0.8 / 64, 0.3 / 64])
    # the most rows
    make("K1024", rng.normal(0, 1, (1024, 64)), 8, 64, [np.linspace(180.0, 220.0, 7)], [np.linspace(0.05, 0.95, 7)], 10)
    _cache["cases"] = c
    return c


def harmonics(case, x=None):
    """The harmonic analysis the module runs in front of the match, by tests/hna_ref.py in float64, rounded to fp32."""
    out = hna_ref.analyse(case["x"] if x is None else x, case["f0"], case["sample_rate"], case["hop"], case["H"])
    return out["amp"].astype(np.float32), out["phase"].astype(np.float32)


def run(case, amp, phase, fp32=False):
    S, N, X = plan(case["table"], case["H"])
    return match(amp, phase, case["f0"], S, N, X, case["sample_rate"], case["n_phi"], fp32=fp32)
