"""CPU: the plain side of the frame-wise filter's ring-kernel tests (tests/ff_ref.py) -- the route table against the host
predicate, the coverage it claims, and that its inputs are fair (the plain fp32 algorithm is well inside the bars) and
discriminate (every wrong oracle is far outside them)."""
import itertools

import numpy as np
import pytest

import ff_ref as R

WORST = {}          # group -> worst emulate_fp32 distance (either norm, any output)


def group(c):
    return c.fwd.split("<")[0]


@pytest.mark.parametrize("c", R.CASES + R.STREAM_CASES, ids=R.case_id)
def test_claimed_labels(c):
    assert (c.fwd, c.bwd) == R.route(c.M, c.hop, c.W)
    assert c.stream == R.stream_route(c.M, c.hop, c.W)


def test_route_agrees_with_the_host_predicate():
    """route() against functional.ff_on_ring_grid over the table and around every rule's edge: orders at the taps of each
    instance, hops at each ring width, windows at multiples of the ring, of 32 and at the backward's LDS limit."""
    from golf_amd.functional import ff_on_ring_grid

    shapes = {(c.M, c.hop, c.W) for c in R.CASES + R.STREAM_CASES}
    orders = sorted({m for _, taps in R.RINGS for m in (taps - 1, taps, taps + 1)} | {1, 64})
    hops = sorted({h for ring, _ in R.RINGS for h in (ring - 1, ring, ring + 1, ring + 4)} | {4, 240, 260})
    for M, hop in itertools.product(orders, hops):
        for ring, _ in R.RINGS:
            for W in (2 * hop, 2 * hop + 2, 4 * hop, -(-2 * hop // ring) * ring, -(-2 * hop // ring) * ring + 32, 96, 960, 1000):
                if W >= 2 * hop:
                    shapes.add((M, hop, W))
    shapes |= {(22, 240, W) for W in (2016, 2040, 2064)} | {(6, 8, W) for W in (2040, 2044, 2048, 4096)}
    shapes |= {(22, 24, W) for W in (14208, 14240, 14272)}      # 4 * (3 * hop + W) around 56 KB (W % 32 == 0)
    assert len(shapes) > 1000
    for M, hop, W in sorted(shapes):
        fwd, bwd = R.route(M, hop, W)
        assert (fwd != "any") == ff_on_ring_grid(M, hop, W, backward=False), (M, hop, W, fwd)
        assert (bwd != "any") == ff_on_ring_grid(M, hop, W, backward=True), (M, hop, W, bwd)
        assert fwd != "any" or bwd == "any"
    assert R.route(22, 24, 14240)[0] == "block<22>" and R.route(22, 24, 14272)[0] == "scalar<24,22>"
    assert R.route(22, 240, 2016) == ("block<22>", "ring<24,22>") and R.route(22, 240, 2040) == ("quad<24,22>", "any")
    # the stream entry: the one-shot's block recursion, else a scalar kernel by the order alone
    assert R.stream_route(22, 16, 64) == "scalar<22>" and R.route(22, 16, 64) == ("any", "any")
    assert R.stream_route(22, 240, 960) == "block<22>" and R.stream_route(7, 250, 1000) == "scalar<14>"
    assert R.stream_route(26, 120, 480) == "scalar<30>" and R.stream_route(38, 8, 16) == "scalar<38>"


def cells(rows):
    fwd = {r[1] for r in rows}
    ring_bwd = {r[2] for r in rows if r[2] != "any"}
    any_behind_ring = {r[1].split("<")[0] for r in rows if r[2] == "any" and r[1] != "any"}
    return fwd, ring_bwd, any_behind_ring, {r[3] for r in rows}


def test_coverage_is_a_stated_fact():
    """Every cell of the routing table is in ROWS, and no row can go without the test noticing."""
    inst = [f"{ring},{taps}" for ring, taps in R.RINGS]
    want_fwd = {f"block<{t}>" for t in (6, 14, 22)} | {f"{k}<{i}>" for k in ("quad", "scalar") for i in inst}
    want_bwd = {f"ring<{i}>" for i in inst}
    want_stream = {f"block<{t}>" for t in (6, 14, 22)} | {f"scalar<{t}>" for _, t in R.RINGS}
    fwd, ring_bwd, any_behind, stream = cells(R.ROWS)
    assert len(want_fwd) == 13 and fwd == want_fwd
    assert ring_bwd == want_bwd
    # the wave-per-frame backward behind a ring forward where W % ring != 0, behind the block recursion and the scalar kernel
    # (its other cause, the 2040-sample LDS limit, is pinned on the predicate: tests/test_ff_anyshape_host.py and above)
    assert any_behind == {"block", "scalar"}
    assert len(want_stream) == 8 and stream == want_stream == {c.stream for c in R.STREAM_CASES}
    # both ends of each instance's order range, and the orders 31 .. 38 that no other test reaches
    for (ring, taps), lo in zip(R.RINGS, (1, 7, 15, 23, 31)):
        orders = {r[0][0] for r in R.ROWS if f"<{ring},{taps}>" in r[1] + r[2] or r[1] == f"block<{taps}>"}
        assert {lo, taps} <= orders, (ring, taps, orders)
    # the three special windows (W = 5 hop, hop > 256, the longest ring<40,38> frame) and the hop that is no ring multiple
    special = {(6, 8, 40), (6, 260, 520), (38, 40, 160), (35, 44, 100)}
    assert len(R.ROWS) == len({r[0] for r in R.ROWS}) == 23 and {r[0] for r in R.ROWS} >= special
    # every row at every count of its tile: 16 +- 1 and 33 frames (quad), 4 +- 1 and 9 (block), 64 +- 1 (b, f) (scalar)
    for shape, fwd_, bwd_, _ in R.ROWS:
        got = {(c.B, c.F) for c in R.CASES if (c.M, c.hop, c.W) == shape}
        assert got == set(R.tile_counts(fwd_)) or (shape[1] == 260 and got == {(3, 17)}), shape
    assert {c.B * R.geometry(c)[2] for c in R.CASES if c.fwd.startswith("scalar")} == {63, 64, 65}
    for chain in ("ring", "any"):
        assert any(c.B * c.F % 4 for c in R.CASES if c.bwd.startswith(chain))


def test_kappa_is_the_kernels_quantity():
    # first order: G[s] = (-a)^(s+1) e_0, the largest row the first for |a| < 1
    assert R.kappa(np.array([0.5]), 6) == 0.5 and R.kappa(np.array([-2.0])) == 2.0 ** 16
    # a zero filter has none; padding with zero taps changes nothing
    assert R.kappa(np.zeros(14), 14) == 0.0
    row = R.draw_rows(np.random.default_rng(0), (1,), 9, 0.7)[0]
    assert R.kappa(row, 14) == pytest.approx(R.kappa(row), rel=1e-14)
    # against the companion matrix: row s of G is e_0^T C^(s+1)
    C = np.zeros((9, 9))
    C[0] = -row
    C[1:, :-1] = np.eye(8)
    P, rows = np.eye(9), []
    for _ in range(16):
        P = P @ C
        rows.append(np.abs(P[0]).sum())
    assert R.kappa(row) == pytest.approx(max(rows), rel=1e-12)


@pytest.mark.parametrize("c", R.CASES + [v for r in R.RAGGED_ROWS for v in R.ragged(r).values()] + R.STREAM_CASES,
                         ids=R.case_id)
def test_inputs_are_fair(c):
    """The plain fp32 algorithm stays within a third of every bar."""
    for k, (emax, el2) in R.distances(R.emulate_fp32(c), R.refs(c)).items():
        frac = max(emax, el2) / R.BARS[k]
        WORST[group(c)] = max(WORST.get(group(c), 0.0), max(emax, el2))
        print(f"{R.case_id(c)} {k}: rel-max {emax:.3e} rel-l2 {el2:.3e}   [worst {group(c)} so far {WORST[group(c)]:.3e}]")
        assert frac <= 1 / 3, (k, emax, el2)


MUTANT_CASES = [R.first_case(shape=r[0]) for r in R.ROWS] + [R.ragged(r)["short"] for r in R.RAGGED_ROWS]


@pytest.mark.parametrize("c", MUTANT_CASES, ids=R.case_id)
def test_inputs_discriminate(c):
    """Every wrong oracle leaves the bar by at least a factor 10 on every output it is meant for."""
    want = R.refs(c)
    for name, mut in R.MUTANTS.items():
        if not mut.meant_for(c):
            continue
        d = R.distances(mut.make(c), want)
        for k in mut.outputs:
            print(f"{R.case_id(c)} {name} {k}: rel-max {d[k][0]:.3e} rel-l2 {d[k][1]:.3e}")
            assert max(d[k]) >= 10 * R.BARS[k], (name, k, d[k])
    assert sum(m.meant_for(c) for m in R.MUTANTS.values()) >= 4


def test_every_mutant_is_used():
    for name, mut in R.MUTANTS.items():
        assert sum(mut.meant_for(c) for c in MUTANT_CASES) >= 4, name


@pytest.mark.parametrize("shape", R.TIER_SHAPES)
def test_planted_tiers(shape):
    """The tier test's frames: kappa a factor four clear of 64 on both sides, the block recursion on the forward, and the
    plain fp32 algorithm within a third of the bars on the planted utterance and on its all-low-wave-1 twin."""
    c, a, a_low, kappas = R.planted(shape)
    assert c.fwd == f"block<{shape[0]}>" and c.bwd.startswith("ring") and c.stream == c.fwd and c.F == 12
    NT = shape[0]
    for f in range(c.F):
        k = R.kappa(a[0, f], NT)
        assert k == kappas[f] and (k >= R.HIGH if f in R.HIGH_FRAMES else k <= R.LOW), (f, k)
    assert R.LOW * 4 == R.KAPPA == R.HIGH / 4
    assert [f for f in range(4, 8) if kappas[f] > R.KAPPA] == [R.SWAPPED]
    assert R.kappa(a_low[0, R.SWAPPED], NT) <= R.LOW and np.array_equal(np.delete(a, R.SWAPPED, 1), np.delete(a_low, R.SWAPPED, 1))
    print(f"{shape}: kappa of the planted frames", " ".join(f"{k:.1f}" for k in kappas[:-1]), f"; swapped in: {kappas[-1]:.1f}")
    for rows in (a, a_low):
        for k, (emax, el2) in R.distances(R.emulate_fp32(c, rows), R.refs(c, rows)).items():
            print(f"{shape} {k}: emulate_fp32 rel-max {emax:.3e} rel-l2 {el2:.3e}")
            WORST["tier"] = max(WORST.get("tier", 0.0), max(emax, el2))
            assert max(emax, el2) <= R.BARS[k] / 3, (k, emax, el2)


def test_zz_worst_emulation_per_group():
    """Not a check: the worst distance of the plain fp32 algorithm per group, for the record (-s shows it)."""
    for g, v in sorted(WORST.items()):
        print(f"worst emulate_fp32 distance, {g}: {v:.3e}")
