/* step_times_san.c -- a stand-alone program for the sanitizers (test_time_plan.py compiles it with
 * csrc/host/solo.c under -fsanitize=address,undefined and runs it): xg_step_times,
 * xg_solo_rail_last, xg_solo_carry_tail and xg_solo_reduce_stamps over seeded random plans of
 * launches, chains and segments, every array allocated at exactly its stated size, so that a read
 * or write one entry past any of them is reported.  Consistent stamps must give ordered times
 * that start after 0 and end at the last mark. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "xg.h"
#include "xg_sched.h"

#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: %s failed (run %d)\n", __FILE__, __LINE__, #x, g_run); \
            exit(1);                                                    \
        }                                                               \
    } while (0)

static int g_run;
static uint64_t g_state = 88172645463325252ull;
static uint64_t rnd(uint64_t n)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return g_state % n;
}

static void one_plan(void)
{
    const int n = 1 + (int)rnd(60);
    uint64_t *marks = malloc(sizeof(uint64_t) * (size_t)(n + 1)), *cst = malloc(sizeof(uint64_t) * (size_t)n);
    uint64_t *est = malloc(sizeof(uint64_t) * (size_t)n);
    int32_t *seg_of = malloc(sizeof(int32_t) * (size_t)n), *chain_end = malloc(sizeof(int32_t) * (size_t)n);
    int32_t *seg_end = malloc(sizeof(int32_t) * (size_t)n);
    uint8_t *need = malloc((size_t)n);
    double *done = malloc(sizeof(double) * (size_t)n);
    CHECK(marks && cst && est && seg_of && chain_end && seg_end && need && done);
    const uint64_t bases[] = {0, 12345, (1ull << 63) + 99, ~0ull - 100000};
    uint64_t t = bases[rnd(4)];      /* wraps past 2^64 for the last base */
    int nseg = 0;
    marks[0] = t;
    for (int s = 0; s < n;) {
        const int kind = (int)rnd(4);
        int e = s + 1;
        if (kind >= 2 && s + 2 <= n) e = s + 2 + (int)rnd((uint64_t)(n - s - 1));
        for (int u = s; u < e; ++u) {
            seg_of[u] = kind == 3 && e - s >= 2 ? nseg : -1;
            chain_end[u] = 0;
            need[u] = (uint8_t)(rnd(10) < 7);
            t += 1 + rnd(100000);
            cst[u] = est[u] = t;
        }
        if (kind == 2 && e - s >= 2) chain_end[s] = e;
        if (kind == 3 && e - s >= 2) seg_end[nseg++] = e;
        t += 50 + rnd(400);
        marks[e] = t;
        s = e;
    }
    need[n - 1] = 1;
    const double hz = rnd(2) ? 1e8 : 2.5e7;
    CHECK(xg_step_times(n, marks, cst, est, seg_of, seg_end, chain_end, rnd(3) ? need : NULL, hz, -1.0, done) == XG_OK);
    CHECK(done[0] > 0);
    for (int s = 1; s < n; ++s) CHECK(done[s] >= done[s - 1]);
    const double end = (double)(marks[n] - marks[0]) / hz;
    CHECK(done[n - 1] == end);
    /* an armed run over the same engine stamps */
    const double total = (double)(est[n - 1] - est[0]) / hz + 1e-6;
    CHECK(xg_step_times(n, NULL, NULL, est, NULL, NULL, NULL, NULL, hz, total, done) == XG_OK);
    CHECK(done[n - 1] == total && done[0] > 0);
    CHECK(xg_step_times(n, marks, NULL, NULL, seg_of, seg_end, NULL, NULL, hz, -1.0, done) == (nseg ? XG_EARG : XG_OK));
    free(marks); free(cst); free(est); free(seg_of); free(chain_end); free(seg_end); free(need); free(done);
}

static void one_segment(void)
{
    const int n = 1 + (int)rnd(30), rails = 1 + (int)rnd(40);
    xg_span *x = malloc(sizeof(xg_span) * (size_t)n);
    int *tb = malloc(sizeof(int) * (size_t)(n + 1));
    CHECK(x && tb);
    uint64_t at = 0;
    for (int t = 0; t < n; ++t) {
        tb[t] = t;
        x[t].src = (1ull << 32) + at;
        x[t].dst = (3ull << 32) + at;
        x[t].len = 1024 * rnd(3 * (uint64_t)rails);      /* often fewer pieces than rails, or none */
        at += x[t].len;
    }
    tb[n] = n;
    x[rnd((uint64_t)n)].len += 1024 * (uint64_t)rails;   /* every rail has a piece */
    xg_solo_shape sh;
    if (xg_solo_tables_g(x, tb, n, rails, 1, 16, 1ull << 32, 3ull << 32, &sh, NULL, NULL) == XG_OK && sh.rails == rails) {
        uint64_t *descs = malloc(sizeof(uint64_t) * (size_t)sh.rails * (size_t)sh.npieces);
        int *meta = malloc(sizeof(int) * (size_t)sh.nmeta);
        int32_t *last = malloc(sizeof(int32_t) * (size_t)rails);
        uint64_t *st = malloc(sizeof(uint64_t) * (size_t)rails * (size_t)n), *out = malloc(sizeof(uint64_t) * (size_t)n);
        CHECK(descs && meta && last && st && out);
        CHECK(xg_solo_tables_g(x, tb, n, rails, 1, 16, 1ull << 32, 3ull << 32, &sh, descs, meta) == XG_OK);
        CHECK(xg_solo_rail_last(x, tb, n, rails, last) == XG_OK);
        const int *cstep = meta + (size_t)rails * (size_t)(sh.nrows + 1);
        for (int r = 0; r < rails; ++r) {
            CHECK(last[r] >= 0 && last[r] < n);
            int s_end = 0;
            for (int k = 0; k < n && cstep[r * n + k] >= 0; ++k) s_end = cstep[r * n + k] + 1;
            CHECK(s_end <= last[r]);          /* the last barrier closes a step before the rail's last */
            for (int t = 0; t < n; ++t) st[(size_t)r * (size_t)n + (size_t)t] = t >= s_end ? 1000 : (uint64_t)(1 + t);
        }
        xg_solo_carry_tail(st, rails, n, 0, n, cstep, last);
        xg_solo_reduce_stamps(st, rails, n, 0, n, out);
        for (int t = 1; t < n; ++t) CHECK(out[t] >= out[t - 1]);
        CHECK(out[n - 1] == 1000);
        free(descs); free(meta); free(last); free(st); free(out);
    }
    free(x); free(tb);
}

int main(void)
{
    /* a plan without steps (a method that posts nothing at -d 0): nothing is read or written */
    const uint64_t start = 7;
    CHECK(xg_step_times(0, &start, NULL, NULL, NULL, NULL, NULL, NULL, 1e8, -1.0, NULL) == XG_OK);
    CHECK(xg_step_times(0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 1e8, 1e-6, NULL) == XG_OK);
    CHECK(xg_step_times(-1, &start, NULL, NULL, NULL, NULL, NULL, NULL, 1e8, -1.0, NULL) == XG_EARG);
    for (g_run = 0; g_run < 2000; ++g_run) {
        one_plan();
        one_segment();
    }
    printf("%d plans timed\n", g_run);
    return 0;
}
