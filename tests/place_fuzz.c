/* Sanitizer fuzz of placement by offset-length lists (csrc/host/place.c) and the tile cut of a
 * copy_kernel_x dispatch (xg_extent_tiles, pieces.c), CPU only: random shapes (P, A, G GPUs, an
 * a2m and an m2a method), random lists -- valid ones, and ones broken in every way xg_exts_check
 * names -- through the check, the length matrix, the schedule, every GPU's placement plan and
 * the tiles of its copies.  A valid list must be accepted and every copy of its plans must lie
 * inside the plan's two regions, the copies' lengths adding up to the hosted extents'; a broken
 * one must be refused with a reason.  Built with the host sources by tests/test_place_host.py under
 * -fsanitize=address,undefined: out-of-bounds bookkeeping, overflow or leaks abort the run. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"

static unsigned long long rng = 0x9E3779B97F4A7C15ull;
static int rnd(int n)
{
    rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17;
    return (int)(rng % (unsigned long long)n);
}

#define FAIL(...) do { fprintf(stderr, __VA_ARGS__); fprintf(stderr, " (list %d)\n", it); return 1; } while (0)

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 200;
    int it, accepted = 0, refused = 0, plans = 0;
    long long tiles = 0;
    for (it = 0; it < iters; ++it) {
        const int P = 2 + rnd(30), A = 1 + rnd(P < 12 ? P : 12), G = 1 + rnd(P < 6 ? P : 6);
        const int method = rnd(2) ? 1 : 2, scatter = method == 1, maxlen = rnd(3) ? 300 : 40000;
        const int64_t n = rnd(400);
        xg_ext *e = (xg_ext *)malloc(sizeof *e * (size_t)(n + 2));
        int64_t *dom = (int64_t *)calloc((size_t)A, sizeof *dom), *lens = (int64_t *)malloc(sizeof *lens * (size_t)P * A);
        int64_t i, total = 0;
        int rl[64], g, rc, brk = rnd(3) == 0 ? 1 + rnd(7) : 0;
        int64_t m = n;
        char err[512];
        if (!e || !dom || !lens) return 2;
        if (xg_aggregator_list(P, A, 1, 1, rl) != 0) FAIL("aggregator list P%d A%d", P, A);
        /* a valid list: every aggregator's extents back to back with gaps, in list order */
        for (i = 0; i < n; ++i) {
            e[i].rank = rnd(P); e[i].agg = rnd(A);
            e[i].len = rnd(4) ? rnd(maxlen) : 0;
            e[i].off = dom[e[i].agg] + (rnd(2) ? rnd(100) : 0);
            dom[e[i].agg] = e[i].off + e[i].len;
            total += e[i].len;
        }
        for (g = 0; g < A; ++g) dom[g] += rnd(64);
        if (brk && n == 0) { e[0].rank = 0; e[0].agg = 0; e[0].off = 0; e[0].len = 1; dom[0] += 1; m = 1; }
        if (brk) {
            const int64_t k = rnd((int)m);
            switch (brk) {
            case 1: e[k].rank = rnd(2) ? P + rnd(3) : -1 - rnd(3); break;
            case 2: e[k].agg = rnd(2) ? A + rnd(3) : -1 - rnd(3); break;
            case 3: e[k].off = -1 - rnd(1000); break;
            case 4: e[k].len = -1 - rnd(1000); break;
            case 5: e[k].off = dom[e[k].agg] - e[k].len + 1 + rnd(50); break;
            case 6: e[k].off = INT64_MAX - rnd(1000); e[k].len = 1001 + rnd(1000); break;
            default:        /* a one-byte overlap (a scatter error only): a second extent on the last byte of one */
                if (e[k].len <= 0) { e[k].len = 1 + rnd(50); if (dom[e[k].agg] < e[k].off + e[k].len) dom[e[k].agg] = e[k].off + e[k].len; }
                e[m].rank = rnd(P); e[m].agg = e[k].agg; e[m].off = e[k].off + e[k].len - 1; e[m].len = 1;
                /* growing e[k] may itself have made an overlap: then the gather case is still legal */
                ++m;
                break;
            }
        }
        rc = xg_exts_check(e, m, P, A, dom, scatter, err, sizeof err);
        if (brk && !(brk == 7 && !scatter)) {
            if (rc != XG_EARG || !err[0]) FAIL("a broken list (kind %d) was accepted or refused without a reason: %d '%s'", brk, rc, err);
            ++refused;
            /* the builders must survive a refused list too: NULL or a plan, no fault */
            if (brk <= 2 && xg_exts_lens(e, m, P, A, lens) != XG_EARG) FAIL("xg_exts_lens took a pair out of range");
            goto next;
        }
        if (brk == 7) {                /* a gather: growing e[k] can only have added overlaps, which are legal */
            if (rc != XG_OK) FAIL("an overlapping list was refused as a gather: %s", err);
        } else if (rc != XG_OK) {
            FAIL("a valid list was refused: %s", err);
        }
        ++accepted;
        if (xg_exts_lens(e, m, P, A, lens) != XG_OK) FAIL("xg_exts_lens refused a checked list");
        {
            int64_t sum = 0, placed = 0, dsum = 0;
            xg_sched *s;
            for (i = 0; i < (int64_t)P * A; ++i) sum += lens[i];
            for (i = 0, total = 0; i < m; ++i) total += e[i].len;
            if (sum != total) FAIL("the matrix sums to %lld, the list to %lld", (long long)sum, (long long)total);
            s = xg_sched_build_v(method, P, A, lens, 3, rl, 1, 1, 0, XG_MPICH_EAGER_LIMIT, 0, err, sizeof err);
            if (!s) FAIL("schedule: %s", err);
            for (g = 0; g < G; ++g) {
                xg_devplan *dp = xg_place_plan_build(s, G, g, e, m, dom);
                int64_t *pl;
                int32_t *begin;
                int k, nt;
                if (!dp) FAIL("xg_place_plan_build returned NULL for GPU %d of %d", g, G);
                ++plans;
                if (dp->nsteps != 1 || dp->np2p != 0 || dp->flags != (XG_DP_RAGGED | XG_DP_EXTENTS) ||
                    dp->steps[0].pre_count != dp->ncopy || dp->steps[0].p2p_count || dp->steps[0].post_count)
                    FAIL("plan shape of GPU %d", g);
                if (dp->region_bytes[scatter ? XG_BUF_RECV : XG_BUF_SEND] != xg_domain_bytes(s, G, g, dom) ||
                    dp->region_bytes[scatter ? XG_BUF_SEND : XG_BUF_RECV] !=
                        xg_region_bytes(s, G, g, scatter ? XG_BUF_RECV : XG_BUF_SEND))
                    FAIL("region sizes of GPU %d", g);
                dsum += xg_domain_bytes(s, G, g, dom);
                pl = (int64_t *)malloc(sizeof *pl * ((size_t)dp->ncopy + 1));
                begin = (int32_t *)malloc(sizeof *begin * ((size_t)dp->ncopy + 2));
                if (!pl || !begin) return 2;
                for (k = 0; k < dp->ncopy; ++k) {
                    const xg_copy *c = &dp->copies[k];
                    if (c->len <= 0 || c->src_buf != XG_BUF_SEND || c->dst_buf != XG_BUF_RECV || c->src_off < 0 ||
                        c->dst_off < 0 || c->src_off + c->len > dp->region_bytes[XG_BUF_SEND] ||
                        c->dst_off + c->len > dp->region_bytes[XG_BUF_RECV])
                        FAIL("copy %d of GPU %d lies outside its regions", k, g);
                    placed += c->len;
                    pl[k] = c->len;
                }
                nt = xg_extent_tiles(pl, dp->ncopy, 16384, 256, begin);
                if (nt < 0 || (dp->ncopy > 0 && (begin[0] != 0 || begin[nt] != dp->ncopy))) FAIL("tiles of GPU %d", g);
                for (k = 0; k < nt; ++k)
                    if (begin[k + 1] <= begin[k] || begin[k + 1] - begin[k] > 256) FAIL("tile %d of GPU %d", k, g);
                tiles += nt;
                free(pl); free(begin);
                xg_devplan_free(dp);
            }
            if (placed != sum) FAIL("the plans place %lld bytes, the list holds %lld", (long long)placed, (long long)sum);
            for (g = 0, i = 0; g < A; ++g) i += dom[g];
            if (dsum != i) FAIL("the GPUs' domain buffers hold %lld bytes, the domains %lld", (long long)dsum, (long long)i);
            xg_sched_free(s);
        }
    next:
        free(e); free(dom); free(lens);
    }
    printf("ok after %d lists: %d accepted, %d refused, %d plans, %lld tiles\n", iters, accepted, refused, plans, tiles);
    return 0;
}
