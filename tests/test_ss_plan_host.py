"""CPU: the launch policy of the sample-wise filter (csrc/lpc_ss_plan.h: make_ss_plan, ss_chain, ss_transitions), walked by a
stand-alone C++ program (tests/ss_plan_host.cpp, built with -fsanitize=address,undefined) over seven shapes x every combination
of HAVE_TRANSITIONS, FAST_TRANSITIONS, SPLIT_P1, FLAT_SCAN, TRAINING, MAPS_ONLY, THROUGHPUT x side stream on/off at 256 CUs.

Checked: the invariants that make a transitions call and the forward that consumes it run the fix-up with the composites
and the zero-state pass exactly once each; literal decisions for the benchmark's shape; the ring table against
functional.SS_RINGS (widths in ascending order); and make_ss_plan's counts and workspace offsets against recorded values
(tests/golden/ss_plan_offsets.json)."""
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

HAVE, FAST, SPLIT_P1, FLAT_SCAN, TRAINING, MAPS_ONLY, THROUGHPUT = 1, 2, 4, 32, 64, 128, 256
M_NONE, M_HAVE, M_OWN, M_WITH_Z, M_VIA = range(5)        # SsMaps
Z_NONE, Z_WITH_MAPS, Z_IN_PREPASS, Z_OWN = range(4)      # SsZeroState
O_NONE, O_PREPASS, O_FIXUP = range(3)                    # SsOwed
N_CU = 256
# (B, T, F, M, hop) -> two-level scan without FLAT_SCAN?  None: no maps (serial; one chunk)
SHAPES = [((32, 47761, 200, 22, 240), True), ((2, 12001, 51, 22, 240), True), ((2, 1201, 6, 22, 240), False),
          ((2, 12001, 51, 30, 240), False), ((48, 47761, 200, 22, 240), False), ((2048, 1201, 6, 22, 240), None),
          ((2, 200, 2, 22, 240), None)]


def _kv(tokens):
    return {k: int(v) for k, v in (t.split("=") for t in tokens)}


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ss_plan") / "ss_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # a stand-alone binary: no runtime to be found at load time
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "golf_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ss_plan_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rings, plans, chains, upw = [], [], [], None
    for line in out.splitlines():
        tok = line.split()
        if tok[0] == "ring":
            rings.append(_kv(tok[1:]))
        elif tok[0] == "plan":
            plans.append(_kv(tok[1:]))
        elif tok[0] == "chain":
            i = tok.index("t:")
            chains.append((_kv(tok[1:i]), _kv(tok[i + 1:])))
        elif tok[0] == "upw":
            upw = [int(v) for v in tok[1:]]
    assert len(plans) == len(SHAPES) and len(chains) == len(SHAPES) * 256
    return {"rings": rings, "plans": plans, "chains": chains, "upw": upw}


def _chain(walk, shape, flags, side=0):
    (c,) = [c for c, _ in walk["chains"] if (c["shape"], c["flags"], c["side"]) == (shape, flags, side)]
    return c


def test_ring_table_matches_functional(walk):
    from golf_amd import functional as GF

    assert tuple((r["W"], r["NT"]) for r in walk["rings"]) == GF.SS_RINGS


def test_plan_offsets_match_recorded(walk):
    recorded = json.load(open(os.path.join(GOLDEN, "ss_plan_offsets.json")))
    assert len(recorded) == len(walk["plans"])
    for (shape, _), want, got in zip(SHAPES, recorded, walk["plans"]):
        assert (want["B"], want["T"], want["F"], want["M"], want["hop"]) == shape
        assert "total" in want and any(k.startswith("off_") for k in want)
        for k, v in want.items():
            assert got[k] == v, (shape, k, got[k], v)
    p = walk["plans"]
    assert (p[0]["NP"], p[0]["NG"]) == (199, 13) and (p[1]["NP"], p[1]["NG"]) == (50, 4) and (p[2]["NP"], p[2]["NG"]) == (5, 0)
    assert (p[3]["W"], p[3]["NT"], p[3]["NG"]) == (40, 32, 0) and p[5]["serial"] == 1 and p[6]["NP"] == 0


def test_chain_invariants(walk):
    plans = walk["plans"]
    for c, t in walk["chains"]:
        p, (shape, two_level) = plans[c["shape"]], SHAPES[c["shape"]]
        flags, side, B = c["flags"], c["side"], shape[0]
        what = (shape, flags, side)
        if two_level is None:   # no maps: nothing to produce, nothing owed
            assert p["has_maps"] == 0 and (c["maps"], c["zero_state"], c["owed"], c["two_level"]) == (M_NONE, Z_NONE, O_NONE, 0), what
            continue
        assert p["has_maps"] == 1 and c["maps"] != M_NONE, what
        # the two-level decision: the plan, B, FLAT_SCAN and the CU count alone -- the backward (its own flags) agrees
        assert c["two_level"] == int(two_level and not flags & FLAT_SCAN), what
        assert c["two_level"] == _chain(walk, c["shape"], flags & FLAT_SCAN)["two_level"] == t["two_level"], what
        # exactly one launch provides the zero-state pass
        assert c["zero_state"] in (Z_WITH_MAPS, Z_IN_PREPASS, Z_OWN), what
        assert (c["zero_state"] == Z_WITH_MAPS) == (c["maps"] == M_WITH_Z), what
        assert (c["zero_state"] == Z_IN_PREPASS) == bool(c["parts"] & 4), what
        # the fix-up and the composites run exactly once across the transitions call and the forward
        own_one_stream = not flags & HAVE and not side and not flags & SPLIT_P1
        owes = own_one_stream or (flags & HAVE and flags & MAPS_ONLY)
        assert (c["owed"] != O_NONE) == bool(owes), what
        # a transitions call ran them iff the forward owes none: the caller's own call (same flags), or launch_transitions inside
        # the forward, which always does
        if flags & HAVE:
            assert (t["owed"] != O_NONE) == (not owes) and (t["owed"] == O_NONE or t["owed"] == (O_PREPASS if t["two_level"] else O_FIXUP)), what
        assert not (c["maps"] == M_VIA and owes), what
        assert (c["maps"] == M_VIA) == (not flags & HAVE and not own_one_stream) and (c["maps"] == M_HAVE) == bool(flags & HAVE), what
        if c["owed"] != O_NONE:
            assert c["owed"] == (O_PREPASS if c["two_level"] else O_FIXUP) and bool(c["parts"] & 1) == bool(c["two_level"]), what
        else:
            assert not c["parts"] & 1, what
        assert (c["fork"], c["join"]) == (int(side and c["maps"] == M_VIA), side), what
        assert (c["fast"], c["training"]) == (int(bool(flags & FAST)), int(not flags & FAST or bool(flags & TRAINING))), what
        scan = ("fast", "training", "two_level", "k1", "k2", "nf", "nu", "nz")   # what fix-up and composites run with: the same in both calls
        assert tuple(t[k] for k in scan) == tuple(c[k] for k in scan), what
        if c["merged"]:
            gxf = -(-p["NC"] // 16)
            assert c["two_level"] and not flags & THROUGHPUT and p["NG"] <= 32 and gxf * (B + -(-B // gxf)) <= 4 * N_CU, what
        if c["zero_state"] == Z_IN_PREPASS:
            assert c["two_level"] and flags & FAST and not side and not flags & SPLIT_P1 and flags & (MAPS_ONLY | THROUGHPUT), what
        if c["two_level"]:
            assert c["parts"] & 2 and (c["nf"], c["nu"], c["nz"]) == (B * (c["k1"] + c["k2"]), B * p["NG"], -(-B * p["NG"] // 4)), what
            k1, k2 = (6, 10) if flags & THROUGHPUT else (10, 38)   # the lone-batch rule; at most one pass over all units
            units = -(-p["NP"] * p["NT"] // 64)
            assert (c["k1"], c["k2"]) == (min(k1, units), min(k2, units - min(k1, units))), what
        else:
            assert (c["merged"], c["thin"], c["parts"]) == (0, 0, 0), what


def test_literal_rows(walk):
    """B 32, T 47761, M 22, hop 240 (NP 199, NG 13): who produces the maps, where the zero-state pass and the fix-up with the
    composites run, the pre-pass `parts` and the chunk-pass form, flag set by flag set; then the same flags at T 1201."""
    def row(flags, side=0, shape=0):
        c = _chain(walk, shape, flags, side)
        return c["maps"], c["zero_state"], c["owed"], c["parts"], c["merged"], c["thin"]

    assert row(FAST) == (M_WITH_Z, Z_WITH_MAPS, O_PREPASS, 3, 1, 0)
    assert row(FAST | THROUGHPUT) == (M_OWN, Z_IN_PREPASS, O_PREPASS, 7, 0, 1)
    assert row(HAVE | FAST) == (M_HAVE, Z_OWN, O_NONE, 2, 1, 0)
    assert row(HAVE | FAST | MAPS_ONLY) == (M_HAVE, Z_IN_PREPASS, O_PREPASS, 7, 1, 0)
    assert row(HAVE | FAST | THROUGHPUT) == (M_HAVE, Z_IN_PREPASS, O_NONE, 6, 0, 1)
    assert row(FAST, side=1) == (M_VIA, Z_OWN, O_NONE, 2, 1, 0) and _chain(walk, 0, FAST, 1)["fork"] == 1
    assert row(FAST | SPLIT_P1) == (M_VIA, Z_OWN, O_NONE, 2, 1, 0) and _chain(walk, 0, FAST | SPLIT_P1)["fork"] == 0
    for flags in (FAST, FAST | TRAINING, 0):   # the transitions call: composites in the pre-pass form, unless MAPS_ONLY
        (t,) = [t for c, t in walk["chains"] if (c["shape"], c["flags"], c["side"]) == (0, flags, 0)]
        (m,) = [t for c, t in walk["chains"] if (c["shape"], c["flags"], c["side"]) == (0, flags | MAPS_ONLY, 0)]
        assert (t["owed"], t["two_level"], m["owed"]) == (O_PREPASS, 1, O_NONE)
    assert row(FAST | FLAT_SCAN) == (M_WITH_Z, Z_WITH_MAPS, O_FIXUP, 0, 0, 0)
    # the same flags at T 1201 (NP 5, NG 0) never give two-level; MAPS_ONLY there still owes the fix-up
    for flags, side in ((FAST, 0), (FAST | THROUGHPUT, 0), (HAVE | FAST, 0), (HAVE | FAST | MAPS_ONLY, 0),
                        (HAVE | FAST | THROUGHPUT, 0), (FAST, 1), (FAST | SPLIT_P1, 0), (FAST | FLAT_SCAN, 0)):
        c = _chain(walk, 2, flags, side)
        assert (c["two_level"], c["merged"], c["thin"], c["parts"]) == (0, 0, 0, 0) and c["zero_state"] != Z_IN_PREPASS
    assert _chain(walk, 2, HAVE | FAST | MAPS_ONLY)["owed"] == O_FIXUP
    assert walk["upw"] == [1, 4, 2]   # 100 + 104 workgroups fit 256 CUs; 250 + 416 / 16 never do; 200 + 52 do with 2 units per wave
