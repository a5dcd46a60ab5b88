"""CPU: the host plan of the block-by-block entries (csrc/stream_plan.h: ring_check_end, ring_plan, frame_position_check,
ring_state_bytes), driven by a stand-alone C++ program (tests/stream_plan_host.cpp, built with -fsanitize=address,undefined)
that reads one case per line and prints one record per case.

Ring model: the schedules a caller can produce over five geometries are walked with a Python model of the carried ring
(slot -> frame) and of the workspace; every accepted call must read its carried frames where the model holds them, form every
output sample from workspace slots that hold the frames covering it, and leave the last min(S, frames so far) frames where the
next call reads them.  A call exactly at each of the four ordering limits passes and is refused, with that limit's text, one
step beyond.  Frame position: frame_position_check against functional._check_frame_position over a grid around every limit."""
import itertools
import os
import random
import re
import subprocess

import pytest
import torch

from conftest import ROOT

GEOMETRIES = ((8, 4), (8, 3), (12, 4), (16, 4), (7, 2))   # (W, hop): S = 1, 2, 2, 3, 3
BIG = 1 << 40


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan",   # a stand-alone binary: no runtime to be found at load time
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "golf_amd", "csrc"),
                    os.path.join(ROOT, "tests", "stream_plan_host.cpp"), "-o", exe], check=True)

    def run(cases):
        """cases: lists of tokens; returns one dict per case (the integers of the record, and msg)."""
        text = "".join(" ".join(str(t) for t in c) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
        assert len(out) == len(cases)
        recs = []
        for line in out:
            head, _, msg = line.partition(" msg=")
            rec = {k: int(v) for k, v in (t.split("=") for t in head.split()[1:] if "=" in t)}
            rec["msg"] = msg
            recs.append(rec)
        return recs

    run.exe = exe
    return run


class Geometry:
    def __init__(self, W, hop, frames):
        self.W, self.hop, self.N, self.pad = W, hop, frames, W // 2
        self.S = -(-W // hop) - 1
        self.Ty = (frames - 1) * hop + W - 2 * self.pad

    def flo(self, n):   # the first frame sample n needs
        d = n + self.pad - self.W + 1
        return 0 if d <= 0 else -(-d // self.hop)

    def finished(self, fdone):   # the samples the first fdone frames finish
        return self.Ty if fdone == self.N else max(0, fdone * self.hop - self.pad)

    def covering(self, n):   # the utterance's frames that reach sample n
        return {g for g in range(self.N) if 0 <= n + self.pad - g * self.hop < self.W}


def schedule(g, take, write_all):
    """The calls (f0, nf, n0, ny, ended) of one utterance: ``take()`` frames per call (clipped to the utterance), and after
    each either all the samples its frames finish or -- where ``write_all()`` is false and the ring still has room -- none.
    The call that filters the last frame has the end markers and writes everything."""
    calls, fdone, ndone = [], 0, 0
    while fdone < g.N or ndone < g.Ty:
        nf = min(take(), g.N - fdone)
        f0, fdone = fdone, fdone + nf
        ended = fdone == g.N
        room = g.flo(ndone) >= fdone - g.S   # writing nothing keeps every frame an unwritten sample needs
        ny = g.finished(fdone) - ndone if ended or write_all() or not room else 0
        calls.append((f0, nf, ndone, ny, ended))
        ndone += ny
    return calls


def schedules(g):
    S = g.S
    for k in sorted({0, 1, 2, S, S + 1}):
        for policy in ("all", "alternate"):
            turn, flip = itertools.count(), itertools.count()
            take = (lambda: next(turn) % 2) if k == 0 else (lambda: k)   # (nothing but empty calls would never end)
            yield f"nf={k} {policy}", schedule(g, take, (lambda: True) if policy == "all" else (lambda: next(flip) % 2 == 1))
    rng = random.Random(1000 * g.W + 10 * g.hop + g.N)
    yield "random", schedule(g, lambda: rng.choice((0, 1, 2, S, S + 1)), lambda: rng.random() < 0.5)


@pytest.mark.parametrize("W,hop", GEOMETRIES)
def test_ring_model(plan, W, hop):
    S = -(-W // hop) - 1
    for frames in (9, 2 * S + 3):
        g = Geometry(W, hop, frames)
        for name, calls in schedules(g):
            recs = plan([("ring", W, hop, f0, nf, n0, ny, g.N if ended else -1, g.Ty if ended else -1, 2, BIG)
                         for f0, nf, n0, ny, ended in calls])
            ring = {}   # slot -> frame
            for (f0, nf, n0, ny, ended), r in zip(calls, recs):
                what = (W, hop, frames, name, (f0, nf, n0, ny, ended), r)
                assert r["rc"] == 0 and r["S"] == S == g.S, what
                assert r["nslot"] == S + nf and r["ncin"] == (min(S, f0) if ny else 0) and r["ncout"] == min(S, nf), what
                ws = [None] * r["nslot"]   # slot -> frame
                for j in range(r["ncin"]):   # the carried frames, from where the model holds them
                    assert ring.get((r["cin_slot"] + j) % S) == f0 - r["ncin"] + j, what
                    ws[S - r["ncin"] + j] = f0 - r["ncin"] + j
                for i in range(nf):
                    ws[S + i] = f0 + i
                for i in range(ny):   # the kernels' frame range of output sample n0 + i
                    m = r["mb"] + i
                    fhi = min(m // hop, r["fmax"])
                    flo = max(0 if m - W + 1 <= 0 else (m - W + hop) // hop, r["fmin"])
                    assert 0 <= r["fmin"] <= flo and fhi <= r["fmax"] < r["nslot"], what
                    assert all(0 <= m - f * hop < W for f in range(flo, fhi + 1)), what
                    read = {ws[f] for f in range(flo, fhi + 1)}
                    assert None not in read and read == g.covering(n0 + i), (what, i, read)
                    assert all(ws[f] == f0 - S + f for f in range(flo, fhi + 1)), what
                for j in range(r["ncout"]):
                    src = r["nslot"] - r["ncout"] + j
                    assert ws[src] == f0 + nf - r["ncout"] + j, what
                    ring[(r["cout_slot"] + j) % S] = ws[src]
                fdone = f0 + nf
                for f in range(fdone - min(S, fdone), fdone):   # where the next call reads them: frame f at slot f % S
                    assert ring.get(f % S) == f, what
            assert calls[-1][4] and calls[-1][2] + calls[-1][3] == g.Ty


@pytest.mark.parametrize("W,hop", GEOMETRIES)
def test_ordering_limits(plan, W, hop):
    g = Geometry(W, hop, 1 << 20)
    S, pad = g.S, g.pad

    def call(f0, nf, n0, ny):
        return ("ring", W, hop, f0, nf, n0, ny, -1, -1, 2, BIG)

    first = (S + 2) * hop - pad                 # where frame S + 2 starts
    keep2 = hop + W - pad                       # the first sample whose earliest frame is 2
    end = lambda fdone: fdone * hop - pad       # the samples fdone frames finish
    cases = [
        # (the call at its limit, one step beyond it, the refusal)
        (call(0, S + 1, 0, end(S + 1)), call(0, S + 1, 0, end(S + 1) + 1), "not filtered yet"),
        (call(S + 2, 2, keep2, end(S + 4) - keep2), call(S + 2, 2, keep2 - 1, end(S + 4) - keep2 + 1), "the carry holds frames from"),
        (call(S + 2, 1, first, hop), call(S + 2, 1, first + 1, hop - 1), "written without frame"),
        (call(S + 2, 1, first, 2 * hop + W - pad - first), call(S + 2, 1, first, 2 * hop + W - pad - first - 1),
         "write the samples up to"),
    ]
    assert g.flo(keep2) == 2 and g.flo(keep2 - 1) == 1 and g.flo(2 * hop + W - pad) == 3 and g.flo(2 * hop + W - pad - 1) == 2
    recs = plan([c for at, beyond, _ in cases for c in (at, beyond)])
    for (at, beyond, text), ok, no in zip(cases, recs[0::2], recs[1::2]):
        assert ok["rc"] == 0, (at, ok)
        assert no["rc"] == -1 and text in no["msg"], (beyond, no)
    # once the utterance has ended, and the workspace
    ended = plan([("ring", W, hop, 0, 3, 0, 0, 2, hop + W - 2 * pad, 2, BIG), ("ring", W, hop, 0, 2, 0, hop + 2, 2, hop + 1, 2, BIG),
                  ("ring", W, hop, 0, 1, 0, 0, -1, -1, 2, 4 * 2 * (S + 1) * W - 1), ("ring", W, hop, 0, 1, 0, 0, -1, -1, 2, 4 * 2 * (S + 1) * W)])
    assert ended[0]["rc"] == -1 and "frames past the last one" in ended[0]["msg"]
    assert ended[1]["rc"] == -1 and "samples past the end" in ended[1]["msg"]
    assert ended[2]["rc"] == -2 and "workspace" in ended[2]["msg"] and ended[3]["rc"] == 0


def test_frame_position_grid_matches_python(plan):
    from golf_amd import functional as GF
    from golf_amd._lib import GolfError

    cases = []
    for hop, (back, ahead, f_back, f_ahead), f_first, n_frames, last in itertools.product(
            (1, 3), ((2, 2, 1, 1), (2, 3, 0, 0)), (0, 1, 3), (1, 2), (0, 1)):
        f_end = f_first + n_frames
        limits = (max(f_first * hop - back, 0), max(f_first - f_back, 0), (f_end - 1) * hop + ahead, f_end + f_ahead)
        for x_t0, f0_first, x_end, f0_end in itertools.product(*[sorted({max(v - 1, 0), v, v + 1}) for v in limits]):
            if x_end - x_t0 >= 0 and f0_end - f0_first >= 1:
                cases.append((x_t0, x_end - x_t0, f0_first, f0_end - f0_first, f_first, n_frames, last, hop, back, ahead, f_back,
                              f_ahead))
    recs = plan([("pos",) + c for c in cases])
    named = re.compile(r"\b(x_t0|f0_first|n_x|n_f0)=")
    refused = 0
    for c, r in zip(cases, recs):
        x_t0, n_x, f0_first, n_f0, f_first, n_frames, last, hop, back, ahead, f_back, f_ahead = c
        try:
            GF._check_frame_position("pos", torch.empty(1, n_x), torch.empty(1, n_f0), x_t0, f_first, f0_first, n_frames, last, hop,
                                     back, ahead, f_back, f_ahead)
            want = None
        except GolfError as e:
            want = named.search(str(e)).group(1)
        if want is None:
            assert r["rc"] == 0, (c, r)
        else:
            refused += 1
            assert r["rc"] == -1 and named.search(r["msg"]).group(1) == want, (c, r, want)
    assert len(cases) > 2000 and 0 < refused < len(cases)


def test_state_bytes(plan):
    out = subprocess.run([plan.exe], input="".join(f"bytes {B} {W} {hop}\n" for W, hop in GEOMETRIES for B in (1, 3)),
                         check=True, capture_output=True, text=True).stdout.split()
    want = [4 * B * (-(-W // hop) - 1) * W for W, hop in GEOMETRIES for B in (1, 3)]
    assert [int(v) for v in out[1::2]] == want
    assert [-(-W // hop) - 1 for W, hop in GEOMETRIES] == [1, 2, 2, 3, 3]
