// Stand-alone walk of csrc/lpc_ss_plan.h for tests/test_ss_plan_host.py: prints the ring table, the plan of every shape and
// the launch chain of every flag combination, one record per line.  Built with -fsanitize=address,undefined.
#include <cstdio>

#include "lpc_ss_plan.h"

using namespace golf;

struct Shape { int B, T, F, M, hop; };
static const Shape kShapes[] = {{32, 47761, 200, 22, 240}, {2, 12001, 51, 22, 240}, {2, 1201, 6, 22, 240}, {2, 12001, 51, 30, 240},
                                {48, 47761, 200, 22, 240}, {2048, 1201, 6, 22, 240}, {2, 200, 2, 22, 240}};
static const int kBits[] = {GOLF_SS_HAVE_TRANSITIONS, GOLF_SS_FAST_TRANSITIONS, GOLF_SS_SPLIT_P1, GOLF_SS_FLAT_SCAN,
                            GOLF_SS_TRAINING, GOLF_SS_MAPS_ONLY, GOLF_SS_THROUGHPUT};

static void print_chain(const SsChain& c) {
    printf(" fast=%d training=%d two_level=%d k1=%d k2=%d nf=%d nu=%d nz=%d maps=%d zero_state=%d owed=%d fork=%d join=%d merged=%d"
           " thin=%d parts=%d", c.fast, c.training, c.two_level, c.k1, c.k2, c.nf, c.nu, c.nz, (int)c.maps, (int)c.zero_state,
           (int)c.owed, c.fork, c.join, c.merged, c.thin, c.parts);
}

int main() {
    const int n_cu = 256;
    for (const WNT& r : kTable) {   // every ring width of the table, once, with its largest NT
        int nt = 0;
        bool first = true;
        for (const WNT& e : kTable) {
            if (e.W == r.W && e.NT > nt) nt = e.NT;
            if (e.W == r.W && &e < &r) first = false;
        }
        if (first) printf("ring W=%d NT=%d\n", r.W, nt);
    }
    int idx = 0;
    for (const Shape& s : kShapes) {
        SsPlan p;
        const bool ok = make_ss_plan(s.B, s.T, s.F, s.M, s.hop, &p);
        printf("plan shape=%d B=%d T=%d F=%d M=%d hop=%d ok=%d W=%d NT=%d L=%d NC=%d NP=%d seg=%d NSEG=%d serial=%d NG=%d GS=%d",
               idx, s.B, s.T, s.F, s.M, s.hop, ok, p.W, p.NT, p.L, p.NC, p.NP, p.seg, p.NSEG, p.serial, p.NG, p.GS);
#define OFF(name) printf(" " #name "=%zu", p.name);
        OFF(off_phi) OFF(off_phiT) OFF(off_z) OFF(off_E) OFF(off_z2) OFF(off_S) OFF(off_zadj) OFF(off_lam) OFF(off_g) OFF(off_pa)
        OFF(off_pg) OFF(off_mt) OFF(off_gv) OFF(off_pmax) OFF(off_tier) OFF(off_S1) OFF(off_status) OFF(off_phi64) OFF(off_fixcnt)
        OFF(off_m64) OFF(off_v64) OFF(off_g64) OFF(off_mtT) OFF(off_L1) OFF(off_wadj) OFF(off_dadj) OFF(off_gflag) OFF(total)
#undef OFF
        printf(" has_maps=%d\n", ss_has_maps(p));
        for (int combo = 0; combo < 1 << 7; ++combo) {
            int flags = 0;
            for (int b = 0; b < 7; ++b)
                if (combo >> b & 1) flags |= kBits[b];
            for (int side = 0; side < 2; ++side) {
                const SsChain c = ss_chain(p, s.B, flags, side != 0, n_cu);
                printf("chain shape=%d flags=%d side=%d", idx, flags, side);
                print_chain(c);
                // the caller's own transitions call with these flags (launch_transitions inside the forward always runs the composites)
                printf(" t:");
                print_chain(ss_transitions(p, s.B, flags, n_cu));
                printf("\n");
            }
        }
        ++idx;
    }
    printf("upw %d %d %d\n", ss_upw(100, 416, n_cu), ss_upw(250, 416, n_cu), ss_upw(200, 416, n_cu));
    return 0;
}
