"""Host checks of tests/harm_ref.py, the plain side of the harmonic bank's edge tests: the float64 closed form against torch
autograd through the dense formula, against the oracle and the goldens; the case table against the launch's host formulas;
every edge the GPU file is meant to run present in the table; functional.upsample_adjoint against the reference's adjoint."""
import numpy as np
import pytest
import torch

import harm_ref as R

GRADS = ("g_phase", "g_amp", "g_tscale", "g_offset", "g_initial_phase")


def _close(got, want, what, tol=1e-10):
    emax, el2 = R.distances(got, want)
    print(f"{what}: rel-max {emax:.2e} rel-l2 {el2:.2e}")
    assert emax <= tol and el2 <= tol, (what, emax, el2)


# ---- the reference itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ops-a1s1h1o1i1", "ops-a0s0h0o0i0", "ops-a0s1h0o1i1", "ends-offset-block", "ends-amp-by1",
                                  "ph37-Tp30", "unvoiced-ph16", "planted", "Tout1", "amp-Fa1", "amp-hop3", "H65"])
def test_reference_agrees_with_float64_autograd(name):
    c = R.case(name)
    d, ref = R.inputs(c), R.refs(c)
    t = {k: None if d[k] is None else torch.tensor(d[k], dtype=torch.float64) for k in
         ("phase", "amp", "tscale", "hscale", "offset", "initial_phase")}
    for k in ("phase", "amp", "tscale", "offset", "initial_phase"):
        if t[k] is not None:
            t[k].requires_grad_(True)
    eps = torch.zeros(c.B, R.geometry(c).Tout, dtype=torch.float64, requires_grad=True)
    y = R.dense_torch(t["phase"], c.H, c.ph, t["amp"], c.ah, t["tscale"], c.sh, t["hscale"], t["offset"], c.oh,
                      t["initial_phase"], eps=eps)
    (dphi,) = torch.autograd.grad(y.sum(), eps, retain_graph=True)
    (y * torch.tensor(d["gy"], dtype=torch.float64)).sum().backward()
    _close(y.detach().numpy(), ref["y"], f"{name} y")
    _close(dphi.numpy(), ref["dphi"], f"{name} dphi")
    seen = 0
    for k in GRADS:
        src = t[k[2:]]
        assert (src is not None) == (k in ref), k
        if src is not None:
            _close(src.grad.numpy(), ref[k], f"{name} {k}")
            seen += 1
    assert seen >= 1


def test_autograd_cases_hold_every_operand():
    c = R.case("ops-a1s1h1o1i1")
    assert c.Fa and c.Fs and c.Fo and c.hs and c.ip
    assert set(R.refs(c)) >= set(R.QUANTITIES)


def test_reference_agrees_with_oracle():
    from oracle import golf_oracle as O

    c = R.case("ops-a1s0h0o1i1")
    d, ref = R.inputs(c), R.refs(c)
    args = (d["phase"], c.ph, d["amp"], c.ah, d["offset"], c.oh, d["initial_phase"])
    _close(ref["y"], O.harmonic_oscillator_forward(*args), "oracle forward (offset, initial_phase)")
    _close(ref["g_offset"], O.harmonic_oscillator_backward_offset(d["gy"], *args), "oracle g_offset")
    _close(ref["g_initial_phase"], O.harmonic_oscillator_backward_initial_phase(d["gy"], *args), "oracle g_initial_phase")
    # the amplitude gradient of the oracle takes the phase and the amplitudes alone: the cases' other operands left out
    for name in ("ops-a1s0h0o0i0", "amp-hop3", "amp-hop300", "amp-hop-beyond", "ph120-Tp9", "long-66tiles"):
        c = R.case(name)
        d = R.inputs(c)
        gy = d["gy"][:, :min(R.up_len(c.Tp, c.ph), R.up_len(c.Fa, c.ah))]
        out = R.harmonic(d["phase"], c.ph, c.H, d["amp"], c.ah, gy=gy)
        _close(out["y"], O.harmonic_oscillator_forward(d["phase"], c.ph, d["amp"], c.ah), f"oracle forward {name}")
        _close(out["g_amp"], O.harmonic_oscillator_backward_amp(gy, d["phase"], c.ph, d["amp"].shape, c.ah),
               f"oracle g_amp {name}")


@pytest.mark.parametrize("tag", ["t", "r", "q"])
def test_reference_reproduces_golden_g18(golden, tag):
    g = golden("g18_harmonic_oscillators")
    amp = g[f"{tag}_amp"]
    out = R.harmonic(g[f"{tag}_phase"], int(g[f"{tag}_phase_hop"]), amp.shape[-1], amp, int(g[f"{tag}_amp_hop"]),
                     gy=g[f"{tag}_gy"])
    _close(out["y"], g[f"{tag}_y"], f"g18{tag} y", 3e-5)
    _close(out["g_amp"], g[f"{tag}_g_amp"], f"g18{tag} g_amp", 3e-5)


@pytest.mark.parametrize("tag", ["t", "r"])
def test_reference_reproduces_golden_g27(golden, tag):
    g = golden("g27_harmonic_phase_terms")
    amp = g[f"{tag}_amp"]
    out = R.harmonic(g[f"{tag}_phase"], int(g[f"{tag}_phase_hop"]), amp.shape[-1], amp, int(g[f"{tag}_amp_hop"]),
                     offset=g[f"{tag}_offset"], po_hop=int(g[f"{tag}_offset_hop"]), initial_phase=g[f"{tag}_initial_phase"],
                     gy=g[f"{tag}_gy"])
    for k in ("y", "g_amp", "g_offset", "g_initial_phase"):
        want = g[f"{tag}_{k}"]
        err = np.abs(out[k] - want).max() / np.abs(want).max()
        print(f"g27{tag} {k}: rel-max {err:.2e}")
        assert out[k].shape == want.shape and err <= 1e-4, (k, err)


# ---- the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_case_claims_match_the_host_formulas(c):
    g = R.geometry(c)
    L = R.lengths(c)
    assert g.Tout == min(L.values()) >= 1
    assert (c.blocks, c.tiles, c.segs, c.ends) == (g.blocks, g.tiles, g.segs, g.ends), (c, g)
    assert g.blocks == -(-g.Tout // 256) and g.tiles == -(-c.Tp // 1024)
    assert g.segs == (max(c.Fa - 1, 1) if c.Fa else 0)
    if c.Fa:
        assert g.nrows == 256 // c.ah + 3
    rows = g.nrows if c.Fa else 1
    assert g.lds == 2080 + 4 * (((c.H + 3) & ~3) + rows * c.H + (2 * c.H if c.ip else 0))
    assert g.lds <= 65536 and R.refusal_of(c.H, c.Fa, c.ah, c.ip) is None, "the table holds only launches the host admits"
    assert c.B <= 3 and c.edge
    if c.grads != "long":
        assert g.Tout <= 4096
    d = R.inputs(c)
    print(f"{c.name}: seed {d['seed']} (+{d['seed'] - c.seed}) margin {d['margin']:.3e}  Tout {g.Tout} blocks {g.blocks} "
          f"tiles {g.tiles} segs {g.segs} lds {g.lds} ends {g.ends}")
    assert d["seed"] - c.seed < R.SEEDS
    assert d["gy"].shape == (c.B, g.Tout)
    if c.voice == "planted":
        agree, near = R.planted_masks_agree(d["phase"], c.H)
        assert c.ph == 1 and agree and near > 0 and d["margin"] <= 2.0 ** -24
    else:
        assert d["margin"] >= R.MARGIN
        assert R.margin_of(d["phase"], c.ph, c.H, g.Tout) == d["margin"]


def test_margin_is_the_brute_force_minimum():
    for name in ("H33", "unvoiced-ph16", "ph37-Tp30"):
        c = R.case(name)
        ref = R.refs(c)
        brute = np.abs(ref["p"][:, :, None] * np.arange(1, c.H + 1) - 0.5).min()
        assert abs(brute - R.margin(c)) <= 1e-15, (name, brute, R.margin(c))
    # a track a seed must be refused for
    assert R.margin_of(np.full((1, 4), 0.1, dtype=np.float64), 1, 5) == 0.0


def test_planted_values():
    c = R.case("planted")
    d, ref = R.inputs(c), R.refs(c)
    p = d["phase"]
    assert p.dtype == np.float32 and set(np.unique(p)) == set(np.float32(R.PLANTED))
    q = ref["p"][0]                     # row 0 holds the values in order, PLANT_RUN samples each
    count = ref["mask"][0].sum(-1)
    want = {0.5: 0, 0.25: 1, 0.125: 3, R.PLANTED[3]: 2, R.PLANTED[4]: 1, R.PLANTED[5]: 2}
    for v, n in want.items():
        assert (count[q == v] == min(n, c.H)).all() and (q == v).sum() == R.PLANT_RUN, (v, n)
    assert R.PLANTED[3] * 3 == 0.5 + 2.0 ** -26 and np.float32(R.PLANTED[3]) * np.float32(3) == np.float32(0.5)
    assert R.PLANTED[4] * 2 == 0.5 + 2.0 ** -24 and R.PLANTED[5] * 2 == 0.5 - 2.0 ** -24
    assert R.planted_masks_agree(np.float32([[0.11]]), 5) == (True, 0)
    # a product that fp32 rounds across 0.5 is told apart: 25 * fp32(0.02) = 0.5 - 6 * 2^-29 in float64, 0.5 in fp32
    lo = np.float32(0.02)
    assert float(lo) * 25 == 0.5 - 6 * 2.0 ** -29 and lo * np.float32(25) == np.float32(0.5)
    assert not R.planted_masks_agree(np.float32([[lo]]), 25)[0] and R.planted_masks_agree(np.float32([[lo]]), 24)[0]


def test_unvoiced_tracks_hold_zeros_and_ramps():
    for name in ("unvoiced-ph16", "unvoiced-ph1"):
        c = R.case(name)
        ref = R.refs(c)
        p, count = ref["p"], ref["mask"].sum(-1)
        assert (p == 0).sum() >= 100 and (count[p == 0] == c.H).all()
        rising = (np.diff(p, axis=1) > 0.2 * p.max() / 16).sum()
        assert rising >= 4 and len(np.unique(count)) >= 10, (name, rising)
        assert (R.inputs(c)["phase"] == 0).any()


def _second_shortest_gap(c):
    L = sorted(R.lengths(c).values())
    return L[1] - L[0] if len(L) > 1 else None


def test_every_edge_is_in_the_table():
    C = R.CASES
    G = {c.name: R.geometry(c) for c in C}
    # operand subsets at one shape, four hops none a multiple of another
    ops = [c for c in C if c.name.startswith("ops-")]
    assert {(bool(c.Fa), bool(c.Fs), c.hs, bool(c.Fo), c.ip) for c in ops} == {
        (a, s, h, o, i) for a in (False, True) for s in (False, True) for h in (False, True) for o in (False, True)
        for i in (False, True)}
    assert len({(c.B, c.H, c.Tp, c.ph, G[c.name].Tout) for c in ops}) == 1 and ops[0].H == 33 and G[ops[0].name].blocks == 3
    full = next(c for c in ops if c.Fa and c.Fs and c.Fo)
    hops = (full.ph, full.ah, full.sh, full.oh)
    assert all(a == b or a % b for a in hops for b in hops) and len(set(hops)) == 4
    # harmonic counts, with the mask cutting below H in some row and at different harmonics
    for H in (1, 31, 32, 33, 64, 65, 155):
        c = next(c for c in C if c.name == f"H{H}")
        count = R.refs(c)["mask"].sum(-1)
        assert c.H == H and c.Fa and c.ip
        if H >= 31:     # a voice cut inside the first anchor block
            assert 0 < count.min() < min(H, 32), (H, np.unique(count))
        if H >= 33:     # and one that runs past it; at 155 the cuts fall in three anchor blocks or more
            assert count.max() > 32 and len(np.unique(count)) >= 3
        if H == 155:
            assert len(np.unique((count - 1) // 32)) >= 3, np.unique(count)
    # which track ends the output: by one sample and by more than a block
    for track in ("phase", "amp", "tscale", "offset"):
        gaps = [_second_shortest_gap(c) for c in C if c.ends == track and c.Fa and c.Fs and c.Fo]
        assert 1 in gaps and any(g > 256 for g in gaps), (track, gaps)
    assert any(c.ends == "phase" and len(R.empty_amp_rows(c)) >= 2 for c in C if c.Fa)
    assert any(c.ends == "offset" and G[c.name].pseudo and G[c.name].Tout > 257 for c in C)
    for T in (1, 2, 255, 256, 257, 258, 512, 513):
        assert any(G[c.name].Tout == T and G[c.name].pseudo for c in C), T
    assert {G[c.name].pseudo[1] for c in C if G[c.name].pseudo and G[c.name].Tout in (257, 258)} == {256}
    # amplitude hops
    amp = [c for c in C if c.Fa]
    assert {1, 3, 7, 100, 255, 256, 257, 300} <= {c.ah for c in amp if G[c.name].blocks >= 3}
    assert any(c.ah > G[c.name].Tout - 1 and c.Fa == 2 and G[c.name].Tout > 256 for c in amp)
    assert any(c.Fa == 1 for c in amp)
    assert any(q > c.Fa - 2 and n < G[c.name].nrows for c in amp for q, _, n in R.staged_rows(c)[-1:])
    assert any(n < G[c.name].nrows and q <= c.Fa - 2 for c in amp for q, _, n in R.staged_rows(c))
    assert any(blk * 256 % c.ah for c in amp for blk in range(1, G[c.name].blocks))
    assert any(c.ah == 1 and c.H == 59 for c in amp)
    assert R.refusal_of(59, 300, 1, True) is None and R.refusal_of(60, 300, 1, False) == "rows"
    # tscale / offset hops
    for hop_of, n_of in ((lambda c: c.sh, lambda c: c.Fs), (lambda c: c.oh, lambda c: c.Fo)):
        have = [c for c in C if n_of(c)]
        assert {1, 3, 7, 100, 255, 256, 257, 300} <= {hop_of(c) for c in have if G[c.name].blocks >= 3}
        assert any(hop_of(c) > G[c.name].Tout - 1 and G[c.name].Tout > 256 for c in have)
        assert any(n_of(c) == 1 and G[c.name].Tout == 1 for c in have)
    # phase hops, frame counts, scan tiles
    assert {1, 2, 37, 120} <= {c.ph for c in C} and {1, 2, 1024, 1025, 2049} <= {c.Tp for c in C}
    long = {c.Tp: c for c in C if c.grads == "long"}
    assert set(long) == {66561, 262144, 262145}
    assert [G[c.name].tiles for c in long.values()] == [66, 256, 257]
    assert all((c.B, c.H, c.ah) == (2, 3, 240) and c.Fa for c in long.values())
    assert all(G[c.name].tiles <= 3 for c in C if c.grads != "long")
    # mask edges
    assert any(c.voice == "planted" and c.ph == 1 and c.Fa for c in C)
    assert {c.ph for c in C if c.voice == "unvoiced"} >= {1, 16}
    # the LDS limit: with initial_phase, the largest H admitted with and without staged amplitude rows
    for Fa, ah in ((0, 1), (3, 256)):
        top = max(H for H in range(1, 4097) if R.refusal_of(H, Fa, ah, True) is None)
        assert any(c.ip and bool(c.Fa) == bool(Fa) and c.ah == ah and c.H == top for c in C), (Fa, ah, top)
        assert R.refusal_of(top + 1, Fa, ah, True) == "lds"
        assert R.lds_bytes_of(top, Fa, ah, True) <= 65536 < R.lds_bytes_of(top + 1, Fa, ah, True)
    # the two launches the issue names, which the row bound alone lets through
    assert R.refusal_of(3000, 3, 256, True) == "lds" and 4 * (4 + 1) * 3000 <= 60 * 1024
    assert R.lds_bytes_of(3000, 3, 256, True) - R.STATIC_LDS == 84000
    assert R.refusal_of(4096, 0, 1, True) == "lds" and R.lds_bytes_of(4096, 0, 1, True) == 65536 + 2080


# ---- upsample_adjoint ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 2, 5, 256])
@pytest.mark.parametrize("F", [1, 2, 4])
def test_upsample_adjoint(hop, F):
    from golf_amd import functional as GF

    full = R.up_len(F, hop)
    M = R.up(np.eye(F)[None], hop)[0].T          # (F, full): row f is frame f's hat function
    assert M.shape == (F, full) and np.allclose(M.sum(0), 1.0)
    rng = np.random.default_rng(hop * 10 + F)
    lens = range(1, full + 1) if full <= 64 else (1, 2, hop, hop + 1, hop + 3, full - 1, full)
    for T in (T for T in lens if 1 <= T <= full):
        v = rng.normal(0, 1, (2, T))
        want = v @ M[:, :T].T
        got = R.up_adjoint(v, hop, F)
        assert np.abs(got - want).max() <= 1e-13, (hop, F, T)
        lib = GF.upsample_adjoint(torch.tensor(v), hop, F).numpy()
        assert lib.shape == (2, F) and np.abs(lib - want).max() <= 1e-13, (hop, F, T)
    v3 = rng.normal(0, 1, (2, full, 3))          # trailing dimensions (the amplitude rows)
    assert np.abs(R.up_adjoint(v3, hop, F) - np.einsum("bth,ft->bfh", v3, M)).max() <= 1e-13


# ---- the library's host check, without a GPU: every call below returns before it launches anything ------------------------
def _entries():
    import ctypes

    from golf_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(256)     # never dereferenced

    def fwd(name, c, Tout, H=None, Fa=None, ah=None, ip=None, Fo=None, ws_bytes=0):
        Fa, ah, ip = c.Fa if Fa is None else Fa, c.ah if ah is None else ah, c.ip if ip is None else ip
        Fo = c.Fo if Fo is None else Fo
        rc = getattr(lib, name)(one, c.Tp, c.Tp, c.ph, one if Fa else None, Fa or 1, ah, one if c.Fs else None, c.Fs or 1, c.sh,
                                None, c.H if H is None else H, one, Tout, c.B, Tout, one, ws_bytes, None,
                                one if Fo else None, Fo or 1, c.oh, one if ip else None)
        return rc, lib.golf_last_error().decode()

    def bwd(c, Tout, Fq, hq, Fo=None):
        Fo = c.Fo if Fo is None else Fo
        rc = lib.golf_harmonic_osc_bwd_amp_f32(one, Tout, one, c.Tp, c.Tp, c.ph, Fq, hq, one if c.Fs else None, c.Fs or 1, c.sh,
                                               None, c.H, one, c.B, Tout, one, 0, None, one if Fo else None, Fo or 1, c.oh,
                                               one if c.ip else None)
        return rc, lib.golf_last_error().decode()

    return fwd, bwd


@pytest.mark.parametrize("c", [c for c in R.CASES if c.grads != "long"], ids=R.case_id)
def test_host_check_admits_every_case(c):
    """Forward, dphase and bwd_amp (with the wrapper's pseudo-frames where initial_phase has no amplitudes) accept the case's
    geometry, whichever track ends the output: they get as far as asking for their workspace (GOLF_EWORKSPACE = -2)."""
    fwd, bwd = _entries()
    g = R.geometry(c)
    for name in ("golf_harmonic_osc_fwd_f32", "golf_harmonic_osc_dphase_f32"):
        rc, msg = fwd(name, c, g.Tout)
        assert rc == -2 and "workspace needs" in msg, (name, rc, msg)
        rc, msg = fwd(name, c, g.Tout + 1)
        assert rc == -1, (name, "one sample more than the shortest track", rc, msg)
    if c.Fa or g.pseudo:
        rc, msg = bwd(c, g.Tout, *((c.Fa, c.ah) if c.Fa else g.pseudo))
        assert rc == -2 and "workspace needs" in msg, (rc, msg)


def test_host_check_refusals():
    fwd, bwd = _entries()
    c = R.case("ends-offset-block")
    g = R.geometry(c)
    for name in ("golf_harmonic_osc_fwd_f32", "golf_harmonic_osc_dphase_f32"):
        # what harm_phase_check refuses stays refused: an offset that does not cover the output asked for
        rc, msg = fwd(name, c, g.Tout, Fo=c.Fo - 1)
        assert rc == -1 and "does not cover" in msg, (rc, msg)
        rc, msg = fwd(name, c, g.Tout - 1)
        assert rc == -1 and "expected" in msg, (rc, msg)
        # the LDS request: the staged-row bound, then the launch's whole request (GOLF_EUNSUPPORTED = -3)
        for H, Fa, ah, ip, edge in ((60, 300, 1, False, True), (3966, 0, 1, True, True), (2267, 3, 256, True, True),
                                    (3000, 3, 256, True, False), (4096, 0, 1, True, False)):
            k = R.case("ops-a0s0h0o0i0")._replace(B=1, Tp=R.up_len(Fa, ah) if Fa else 300, ph=1)
            T = R.up_len(k.Tp, 1)
            assert R.refusal_of(H, Fa, ah, ip)
            rc, msg = fwd(name, k, T, H=H, Fa=Fa, ah=ah, ip=ip)
            assert rc == -3 and "LDS staging" in msg and "harmonics" in msg, (H, Fa, ah, ip, rc, msg)
            if edge:   # one harmonic fewer is admitted
                rc, msg = fwd(name, k, T, H=H - 1, Fa=Fa, ah=ah, ip=ip)
                assert rc == -2 and R.refusal_of(H - 1, Fa, ah, ip) is None, (H - 1, Fa, ah, ip, rc, msg)
    rc, msg = bwd(c, g.Tout, c.Fa, c.ah, Fo=c.Fo - 1)
    assert rc == -1 and "does not cover" in msg, (rc, msg)
    rc, msg = bwd(c, g.Tout - 1, c.Fa, c.ah)
    assert rc == -1 and "expected" in msg, (rc, msg)
