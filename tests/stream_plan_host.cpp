// Stand-alone driver of csrc/stream_plan.h for tests/test_stream_plan_host.py: reads one case per line from stdin and prints
// one record per case.  Built with -fsanitize=address,undefined.
//   ring W hop f0 nf n0 ny nfr Ty B ws_bytes   (nfr < 0: the utterance has not ended)
//   pos x_t0 n_x f0_first n_f0 f_first n_frames last hop back ahead f_back f_ahead
//   bytes B W hop
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "stream_plan.h"

static char g_msg[512];

namespace golf {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace golf

using namespace golf;

int main() {
    char kind[16];
    while (scanf("%15s", kind) == 1) {
        g_msg[0] = 0;
        if (!strcmp(kind, "ring")) {
            int W, hop, nf, ny, B;
            long long f0, n0, nfr, Ty, ws_bytes;
            if (scanf("%d %d %lld %d %lld %d %lld %lld %d %lld", &W, &hop, &f0, &nf, &n0, &ny, &nfr, &Ty, &B, &ws_bytes) != 10) return 2;
            const bool fin = nfr >= 0;
            RingPlan p = {};
            int rc = fin ? ring_check_end("ring", f0, nf, n0, ny, nfr, Ty) : GOLF_OK;
            if (rc == GOLF_OK)
                rc = ring_plan("ring", W, hop, f0, nf, n0, ny, fin ? nfr : kRingOpen, fin ? Ty : kRingOpen, B, (const void*)256,
                               (size_t)ws_bytes, &p);
            printf("ring rc=%d S=%d ncin=%d cin_slot=%d ncout=%d cout_slot=%d nslot=%d mb=%d fmin=%d fmax=%d msg=%s\n", rc,
                   ring_S(W, hop), p.ncin, p.cin_slot, p.ncout, p.cout_slot, p.nslot, p.mb, p.fmin, p.fmax, g_msg);
        } else if (!strcmp(kind, "pos")) {
            long long x_t0, f0_first, f_first, back, ahead;
            int n_x, n_f0, n_frames, last, hop, f_back, f_ahead;
            if (scanf("%lld %d %lld %d %lld %d %d %d %lld %lld %d %d", &x_t0, &n_x, &f0_first, &n_f0, &f_first, &n_frames, &last, &hop,
                      &back, &ahead, &f_back, &f_ahead) != 12)
                return 2;
            const int rc = frame_position_check("pos", x_t0, n_x, f0_first, n_f0, f_first, n_frames, last, hop, back, ahead, f_back,
                                                f_ahead);
            printf("pos rc=%d msg=%s\n", rc, g_msg);
        } else if (!strcmp(kind, "bytes")) {
            int B, W, hop;
            if (scanf("%d %d %d", &B, &W, &hop) != 3) return 2;
            printf("bytes %zu\n", ring_state_bytes(B, W, hop));
        } else {
            return 2;
        }
    }
    return 0;
}
