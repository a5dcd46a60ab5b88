"""CPU: HarmonicPlusNoiseStream's bookkeeping (pure host functions of the pushed lengths, checked against float64 oracle
compositions of the ddsp, sawsing, pulse and glottal_d decoders), its refusals, and the argument checks of the streaming
harmonic oscillator entry (no launch)."""
import numpy as np
import pytest

# the decoders of the shipped configs HarmonicPlusNoiseStream covers (tests/golden/g28_shipped_configs.npz), with the hops the
# vocoders feed them: interspeech24 DDSP at hop 240 with a per-sample phase, the ISMIR'23 models at hop 120 with the phase at
# hop 120 and a voicing track
SPECS = {
    "ddsp": dict(rel="ckpts/interspeech24/ddsp/config.yaml", P=1, hop=240, amp=155, noise=("fir", 256), room=True),
    "ddsp_f1": dict(rel="ckpts/ismir23/ddsp_f1/config.yaml", P=120, hop=120, amp=150, noise=("fir", 80), voicing=True),
    "sawsing": dict(rel="ckpts/ismir23/sawsing_f1/config.yaml", P=120, hop=120, harm=("fir", 256), noise=("fir", 80),
                    voicing=True),
    "pulse": dict(rel="ckpts/ismir23/pulse_f1/config.yaml", P=120, hop=120, harm=("frames", 26), noise=("frames", 22),
                  voicing=True),
    "glottal_d": dict(rel="ckpts/ismir23/glottal_d_f1/config.yaml", P=120, hop=120, wsel=1200, harm=("frames", 22),
                      noise=("frames", 22), voicing=True),
}


def shipped(golden, name):
    from golf_amd.config import build_model

    g = golden("g28_shipped_configs")
    paths = list(g["path"])
    m = build_model(str(g["config"][paths.index(SPECS[name]["rel"])]))
    return getattr(m, "decoder", m)


def geometry(name, dec):
    """The HPNGeometry HarmonicPlusNoiseStream derives for this decoder and these hops."""
    from golf_amd.stream import BranchGeometry, HPNGeometry

    s = SPECS[name]

    def branch(kind, f):
        if kind is None:
            return BranchGeometry()
        if kind[0] == "fir":
            return BranchGeometry("fir", hop=s["hop"], taps=2 * (kind[1] - 1))
        return BranchGeometry("frames", hop=s["hop"], window=int(f._window.numel()), centred=bool(f.centred))

    kw = dict(source="glottal", w_hop=s["wsel"]) if "wsel" in s else dict(amp_hop=s["hop"] if "amp" in s else 0)
    return HPNGeometry(phase_hop=s["P"], harm=branch(s.get("harm"), dec.harm_filter),
                       noise=branch(s.get("noise"), dec.noise_filter), **kw)


def make_hpn_inputs(name, B, T, seed=2434, device="cpu"):
    """Control tracks for decoder ``name``: phase (and voicing) at the phase hop, amplitudes / table select, each branch's
    controls, noise (B, T) and the room kernel."""
    import torch

    from golf_amd.synthetic import make_harmonic_amplitudes, make_inputs

    s = SPECS[name]
    hop, P = s["hop"], s["P"]
    lpc_m = lambda k: k[1] if k and k[0] == "frames" else 22
    n_mag = lambda k: k[1] if k and k[0] == "fir" else 256
    a = make_inputs(B=B, T=T, hop=hop, M=lpc_m(s.get("harm")), seed=seed, with_noise_filter=True, n_mag=n_mag(s.get("harm")))
    b = make_inputs(B=B, T=T, hop=hop, M=lpc_m(s.get("noise")), seed=seed + 1, with_noise_filter=True,
                    n_mag=n_mag(s.get("noise")))
    ctrl = lambda k, d: () if k is None else ((d["log_mag"],) if k[0] == "fir" else (d["gain"], d["a"]))
    x = dict(phase=a["phase"][:, ::P].contiguous(), noise=a["noise"], room_kernel=a["room_kernel"],
             harm=ctrl(s.get("harm"), a), noise_ctrl=ctrl(s.get("noise"), b), F=a["gain"].shape[1])
    if "amp" in s:
        x["amp"] = make_harmonic_amplitudes(B, x["F"], s["amp"], seed=seed)
    if "wsel" in s:
        F_w = (T - 1) // s["wsel"] + 2
        x["wsel"] = a["wsel"][:, :F_w].contiguous() if a["wsel"].shape[1] >= F_w else \
            torch.sigmoid(torch.cumsum(0.3 * torch.randn(B, F_w, generator=torch.Generator().manual_seed(seed)), 1))
    if s.get("voicing"):
        g = torch.Generator().manual_seed(seed + 2)
        x["voicing"] = torch.sigmoid(2 + torch.cumsum(0.4 * torch.randn(B, x["phase"].shape[1], generator=g), 1))
    out = {}
    for k, v in x.items():
        if isinstance(v, tuple):
            out[k] = tuple(t.to(device) for t in v)
        else:
            out[k] = v.to(device) if hasattr(v, "to") else v
    return out


def compose(name, dec, x):
    """The one-shot decoder as the float64 oracle composes it, on numpy float64 tracks ``x`` (make_hpn_inputs' keys)."""
    from oracle import golf_oracle as O

    s = SPECS[name]
    P, hop = s["P"], s["hop"]
    ph = x["phase"]
    if "voicing" in x:
        n = min(ph.shape[1], x["voicing"].shape[1])
        ph = ph[:, :n] * x["voicing"][:, :n]
    osc = dec.harm_oscillator
    kind = type(osc).__name__
    sc = 1.0 / np.sqrt(0.5 / ph)
    if "wsel" in s:
        src = O.indexed_glottal_forward(ph, P, x["wsel"], s["wsel"], osc.table.double().numpy(), 1, bool(osc.equal_energy))["out"]
    else:
        B, Tp = ph.shape
        if kind == "AdditiveSynthesizer" and P == 1:
            A = O.linear_upsample(x["amp"], hop, axis=1)
            n = min(A.shape[1], Tp)
            amps, ahop = A[:, :n] * sc[:, :n, None], 1
        elif kind == "AdditiveSynthesizer":
            n = min(x["amp"].shape[1], Tp)
            amps, ahop = x["amp"][:, :n] * sc[:, :n, None], P
        elif kind == "V1AdditiveSynthesizer":
            amps, ahop = x["amp"], hop
        elif kind == "SawToothOscillator":
            amps, ahop = np.broadcast_to(osc.amplitudes.double().numpy(), (B, Tp, osc.amplitudes.numel())), P
        else:
            amps, ahop = np.repeat(sc[:, :, None], osc.num_harmonics, 2), P
        src = O.harmonic_oscillator_forward(ph, P, amps, ahop)
    noise = x["noise"][:, : src.shape[1]]

    def branch(f, kind, v, ctrl):
        if kind is None:
            return v
        if kind[0] == "fir":
            N = 2 * (kind[1] - 1)
            return O.ltv_fir_frames_forward(v, O.zero_phase_fir_kernels(ctrl[0], f._window(N, "cpu").double().numpy()), hop)
        return O.lti_frames_ola_forward(v, ctrl[0], ctrl[1], hop, f._window.double().numpy(), centred=bool(f.centred))[0]

    yh = branch(dec.harm_filter, s.get("harm"), src, x["harm"])
    yn = branch(dec.noise_filter, s.get("noise"), noise, x["noise_ctrl"])
    n = min(yh.shape[1], yn.shape[1])
    y = yh[:, :n] + yn[:, :n]
    return O.lti_acoustic_filter_forward(y, x["room_kernel"]) if s.get("room") else y


def _np(x):
    return {k: (tuple(t.double().numpy() for t in v) if isinstance(v, tuple) else
                (v.double().numpy() if hasattr(v, "double") else v)) for k, v in x.items()}


def _flat(x):
    """(key, tensor) of every pushed track: tuples become key0, key1."""
    out = {}
    for k, v in x.items():
        if isinstance(v, tuple):
            out.update({f"{k}{i}": t for i, t in enumerate(v)})
        elif k not in ("room_kernel", "F"):
            out[k] = v
    return out


def _unflat(d, like):
    x = dict(like)
    for k, v in like.items():
        if isinstance(v, tuple):
            x[k] = tuple(d[f"{k}{i}"] for i in range(len(v)))
        elif k in d:
            x[k] = d[k]
    return x


def _emit(g, name, n):
    from golf_amd.stream import hpn_emit_count

    n_phase = min(n["phase"], n["voicing"]) if "voicing" in n else n["phase"]
    n_src = n["wsel"] if "wsel" in n else n.get("amp")
    ctrl = lambda k: tuple(n[kk] for kk in sorted(n) if kk.startswith(k) and kk[len(k):].isdigit())
    return hpn_emit_count(g, n_phase, n_src, n["noise"], ctrl("harm"), ctrl("noise_ctrl"))


@pytest.mark.parametrize("name", ["ddsp", "sawsing", "pulse", "glottal_d"])
def test_emitted_samples_depend_only_on_pushed_inputs(golden, name):
    """For random push prefixes, every input step not yet pushed is replaced by other values (lengths kept): the first
    hpn_emit_count(...) samples of the oracle composition do not move, and the final length is the composition's."""
    from golf_amd.stream import hpn_final_lengths

    dec = shipped(golden, name)
    g = geometry(name, dec)
    T = 7200 if SPECS[name]["P"] == 1 else 9600
    base, other = _np(make_hpn_inputs(name, 1, T)), _np(make_hpn_inputs(name, 1, T, seed=7))
    ref = compose(name, dec, base)
    fb = _flat(base)
    n_all = {k: v.shape[1] for k, v in fb.items()}
    hc = tuple(t.shape[1] for t in base["harm"])
    nc = tuple(t.shape[1] for t in base["noise_ctrl"])
    n_phase = min(n_all["phase"], n_all.get("voicing", n_all["phase"]))
    src = n_all["wsel"] if "wsel" in n_all else n_all.get("amp")
    assert hpn_final_lengths(g, n_phase, src, T, hc, nc)["out"] == ref.shape[1]
    rng = np.random.default_rng(5)
    checked = 0
    for it in range(8):
        if it % 2:   # everything up to one input time, the way a live stream pushes
            S = int(rng.integers(0, T))
            hops = dict(phase=SPECS[name]["P"], voicing=SPECS[name]["P"], amp=SPECS[name]["hop"], wsel=SPECS[name].get("wsel"),
                        noise=1)
            n = {k: min(S // hops.get(k, SPECS[name]["hop"]) + 1, v) for k, v in n_all.items()}
        else:
            n = {k: int(rng.integers(0, v + 1)) for k, v in n_all.items()}
        E = _emit(g, name, n)
        fo = _flat(other)
        mod = _unflat({k: np.concatenate([fb[k][:, : n[k]], fo[k][:, n[k]:]], 1) for k in fb}, base)
        y = compose(name, dec, mod)
        assert y.shape == ref.shape
        if E:
            err = np.abs(y[:, :E] - ref[:, :E]).max() / np.abs(ref).max()
            assert err <= 1e-12, (n, E, err)
            checked += 1
    assert checked >= 2


def _first_time(E, t, lo, hi):
    if E(hi) <= t:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if E(mid) > t:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("name", list(SPECS))
def test_latency_formula_is_a_bound_and_tight(golden, name):
    """Every track pushed up to input time S: output t is out by S = t + latency at the latest, and some t needs more than
    latency - hop."""
    from golf_amd.stream import hpn_emit_count, hpn_stream_latency

    dec = shipped(golden, name)
    g = geometry(name, dec)
    s = SPECS[name]
    L = hpn_stream_latency(g)
    hop, P = s["hop"], s["P"]
    nh = 2 if g.harm.kind == "frames" else (1 if g.harm.kind == "fir" else 0)
    nn = 2 if g.noise.kind == "frames" else (1 if g.noise.kind == "fir" else 0)

    def E(S):
        src = S // s["wsel"] + 1 if "wsel" in s else (S // hop + 1 if "amp" in s else None)
        return hpn_emit_count(g, S // P + 1, src, S + 1, (S // hop + 1,) * nh, (S // hop + 1,) * nn)

    worst = 0
    for t in range(0, 6 * max(hop, s.get("wsel", 0), P) + 1, 7 if P == 1 else 1):
        need = _first_time(E, t, t, t + L)
        assert need is not None, (name, t, L)
        worst = max(worst, need - t)
    assert L - hop < worst <= L, (name, worst, L)


@pytest.mark.parametrize("name", list(SPECS))
def test_final_lengths_match_the_one_shot_modules(golden, name):
    """hpn_final_lengths against the lengths the one-shot modules produce (CPU-only arithmetic of each module)."""
    from golf_amd import functional as GF
    from golf_amd.stream import hpn_final_lengths

    dec = shipped(golden, name)
    g = geometry(name, dec)
    s = SPECS[name]
    P, hop = s["P"], s["hop"]
    for T in (4801, 7199, 7200, 12345, 48000):
        Tp = (T - 1) // P + 1
        N = (Tp - 1) * P + 1 if P > 1 else Tp
        for F in (T // hop - 3, T // hop + 1, T // hop + 5):
            for n_noise in (None, T - 700):
                src_rows = (T - 1) // s["wsel"] + 2 if "wsel" in s else (F if "amp" in s else None)
                if "amp" in s and P > 1:   # AdditiveSynthesizer folds the scale in: rows = min(F, Tp)
                    S = min(N, (min(F, Tp) - 1) * hop + 1)
                    src_rows = min(F, Tp) if type(dec.harm_oscillator).__name__ == "AdditiveSynthesizer" else F
                    S = min(N, (src_rows - 1) * hop + 1)
                elif "amp" in s:
                    S = min(N, (F - 1) * hop + 1)
                else:
                    S = N
                noise = S if n_noise is None else min(n_noise, S)

                def branch(b, n_in):
                    if b.kind == "pass":
                        return n_in
                    if b.kind == "fir":
                        return GF.fir_frames_length(n_in, F, b.taps, b.hop)
                    Tx, nfr, Ty = GF.ff_output_length(n_in - b.shift, F, b.hop, b.window)
                    return None if nfr > F else Ty + b.shift

                yh, yn = branch(g.harm, S), branch(g.noise, noise)
                if yh is None or yn is None:
                    continue
                nh = {"pass": 0, "fir": 1, "frames": 2}
                fl = hpn_final_lengths(g, Tp, src_rows, n_noise, (F,) * nh[g.harm.kind], (F,) * nh[g.noise.kind])
                assert fl["source"] == S and fl["noise"] == noise, (T, F)
                assert fl["out"] == min(yh, yn), (name, T, F, n_noise, fl, yh, yn)


def test_refusals(golden):
    import torch

    from golf_amd.audiotensor import AudioTensor
    from golf_amd.filters import LTVMinimumPhaseFilterPrecise, LTVZeroPhaseFIRFilterPrecise
    from golf_amd.noise import UniformNoise
    from golf_amd.stream import FramewiseDecoderStream, HarmonicPlusNoiseStream, open_stream
    from golf_amd.synth import PulseTrain
    from golf_amd.synthetic import make_ddsp_decoder, make_decoder

    # the existing classes and open_stream keep their refusals
    with pytest.raises(NotImplementedError, match="AdditiveSynthesizer"):
        open_stream(make_ddsp_decoder(), 2)
    d = shipped(golden, "pulse")
    with pytest.raises(NotImplementedError, match="AdditivePulseTrain"):
        FramewiseDecoderStream(d, 2)
    # every decoder of the table opens
    for name in SPECS:
        HarmonicPlusNoiseStream(shipped(golden, name), 2)
    HarmonicPlusNoiseStream(make_ddsp_decoder(), 2)
    with pytest.raises(NotImplementedError, match="SourceFilterSynth"):
        HarmonicPlusNoiseStream(make_decoder(), 2)
    d = make_ddsp_decoder()
    d.noise_generator = UniformNoise()
    with pytest.raises(NotImplementedError, match="UniformNoise"):
        HarmonicPlusNoiseStream(d, 2)
    d = make_ddsp_decoder()
    d.noise_filter = LTVZeroPhaseFIRFilterPrecise(window="hanning", n_mag=256)
    with pytest.raises(NotImplementedError, match="LTVZeroPhaseFIRFilterPrecise"):
        HarmonicPlusNoiseStream(d, 2)
    d = make_ddsp_decoder()
    d.harm_filter = LTVMinimumPhaseFilterPrecise(lpc_order=22)
    with pytest.raises(NotImplementedError, match="sample-wise LPC"):
        HarmonicPlusNoiseStream(d, 2)
    d = make_ddsp_decoder()
    d.end_filter = LTVZeroPhaseFIRFilterPrecise(window="hanning", n_mag=256)
    with pytest.raises(NotImplementedError, match="end filter"):
        HarmonicPlusNoiseStream(d, 2)
    d = make_ddsp_decoder()
    d.harm_oscillator = PulseTrain()
    with pytest.raises(NotImplementedError, match="PulseTrain"):
        HarmonicPlusNoiseStream(d, 2)
    # push-time refusals (all before any device work)
    z = lambda *s, hop=1: AudioTensor(torch.zeros(*s), hop)
    st = HarmonicPlusNoiseStream(make_ddsp_decoder(), 2)
    args = dict(phase=z(2, 1), harm_oscillator_params=(z(2, 1, 155, hop=240),), noise_filter_params=(z(2, 1, 256, hop=240),))
    with pytest.raises(NotImplementedError, match="voicing at hop 240"):
        st.push(**args, voicing=z(2, 1, hop=240))
    with pytest.raises(NotImplementedError, match="requires grad"):
        st.push(**{**args, "phase": AudioTensor(torch.zeros(2, 1, requires_grad=True))})
    with pytest.raises(NotImplementedError, match="initial_phase"):
        st.push(**{**args, "harm_oscillator_params": args["harm_oscillator_params"] + (z(2, 155),)})
    with pytest.raises(ValueError, match="noise_filter_params"):
        st.push(**{**args, "noise_filter_params": ()})
    with pytest.raises(Exception, match="ROCm device"):   # CPU tensors: there is no CPU path
        st.push(**args)
    st = HarmonicPlusNoiseStream(make_ddsp_decoder(), 2)
    with pytest.raises(NotImplementedError, match="AdditiveSynthesizer with the phase at hop 120"):
        st.push(phase=z(2, 1, hop=120), harm_oscillator_params=(z(2, 1, 155, hop=240),),
                noise_filter_params=(z(2, 1, 256, hop=240),))


def test_stream_entry_refuses_bad_arguments_without_launch():
    import ctypes

    from golf_amd import _lib

    lib = _lib.load()
    f = lib.golf_harmonic_osc_stream_f32
    one = ctypes.c_void_p(256)   # never dereferenced: every call below is refused on its arguments
    # a valid call: segments 10..19 at phase hop 1 (samples 10..19), amplitude rows 0..1 at hop 240 (open), tscale rows 10..20
    ok = dict(phase=one, phase_stride=11, nseg=10, final_point=0, phase_hop=1, amp=one, a_first=0, na=2, a_end=-1,
              amp_hop=240, tscale=one, ts_stride=11, s_first=10, ns=11, s_end=-1, ts_hop=1, hscale=None, H=155, j0=10,
              acc=one, out=one, out_stride=10, B=2, ws=one, ws_bytes=1 << 20, stream=None)
    names = list(ok)

    def refused(match, code=-1, **kw):
        rc = f(*[kw.get(k, ok[k]) for k in names])
        assert rc == code, (kw, rc, lib.golf_last_error())
        assert match.encode() in lib.golf_last_error(), (kw, lib.golf_last_error())

    refused("null", phase=None)
    refused("null", acc=None)
    refused("null", out=None)
    refused("bad size", H=4097)
    refused("bad size", H=0)
    refused("bad size", final_point=2)
    refused("bad size", j0=-1)
    refused("stride", phase_stride=10)
    refused("stride", out_stride=9)
    refused("amplitude rows", na=1)                       # sample 19 interpolates rows 0 and 1
    refused("amplitude rows", a_first=1)
    refused("amplitude rows", a_end=1)                    # a closed single row reaches sample 0 only
    refused("amplitude rows", a_end=2, amp_hop=5)         # a closed track that ends before sample 19 (the one-shot's Tout: 6)
    refused("tscale rows", s_first=11, ns=10)
    refused("tscale rows", ns=10, ts_stride=10)           # sample 19 needs row 20
    refused("tscale rows", ts_stride=5)
    refused("too fine", code=-3, amp_hop=1, na=30, H=4096)   # the one-shot's LDS staging limit, its error class
    refused("workspace", code=-2, ws_bytes=8 * 2 * 10 - 1)
    # nothing to do is not an error and launches nothing
    assert f(*[dict(ok, nseg=0, out=None, ws=None, ws_bytes=0)[k] for k in names]) == 0
