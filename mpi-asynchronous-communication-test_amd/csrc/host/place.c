/*
 * place.c -- placement of exchanged segments by offset-length lists (include/xg_sched.h).
 *
 * In ROMIO's two-phase I/O the bytes a rank sends to an aggregator land in the aggregator's
 * collective buffer (its file domain) as a list of offset-length pairs (others_req[i].offsets /
 * lens, posted as an hindexed type); a collective read gathers such a list out of the domain.
 * Here the list is checked (xg_exts_check), turned into the length matrix of the exchange
 * (xg_exts_lens) and into one GPU-local copy step -- a device plan of one copy per extent between
 * the exchange's dense layout and the GPU's domain buffer (xg_place_plan_build) -- which runs
 * after the exchange (a2m: scatter) or before it (m2a: gather).
 */
#include "sched_int.h"
#include "xg.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int pair_ok(const xg_ext *e, int procs, int cb_nodes)
{
    return e->rank >= 0 && e->rank < procs && e->agg >= 0 && e->agg < cb_nodes;
}

int xg_exts_lens(const xg_ext *exts, int64_t n, int procs, int cb_nodes, int64_t *lens)
{
    int64_t i;
    if (procs <= 0 || cb_nodes <= 0 || !lens || n < 0 || (n && !exts)) return XG_EARG;
    memset(lens, 0, sizeof(int64_t) * (size_t)procs * (size_t)cb_nodes);
    for (i = 0; i < n; ++i) {
        int64_t *l;
        if (!pair_ok(&exts[i], procs, cb_nodes) || exts[i].len < 0) return XG_EARG;
        l = &lens[(size_t)exts[i].rank * cb_nodes + exts[i].agg];
        if (*l > INT64_MAX - exts[i].len) return XG_EARG;
        *l += exts[i].len;
    }
    return XG_OK;
}

typedef struct { int64_t lo, hi, at; } span_t;       /* [lo, hi) of a domain, list index `at` */

static int span_cmp(const void *x, const void *y)
{
    const span_t *a = (const span_t *)x, *b = (const span_t *)y;
    if (a->lo != b->lo) return a->lo < b->lo ? -1 : 1;
    return a->at < b->at ? -1 : a->at > b->at;
}

int xg_exts_check(const xg_ext *exts, int64_t n, int procs, int cb_nodes, const int64_t *dom_bytes, int scatter,
                  char *err, size_t errlen)
{
    char ebuf[8];
    int64_t i, *cnt = NULL, *beg = NULL;
    span_t *sp = NULL;
    int a, rc = XG_OK;
    if (!err) { err = ebuf; errlen = sizeof ebuf; }
    if (errlen) err[0] = 0;
    if (procs <= 0 || cb_nodes <= 0 || n < 0 || (n && !exts) || !dom_bytes) {
        snprintf(err, errlen, "extent list: bad arguments (procs %d, cb_nodes %d, n %lld)", procs, cb_nodes,
                 (long long)n);
        return XG_EARG;
    }
    for (a = 0; a < cb_nodes; ++a)
        if (dom_bytes[a] < 0) {
            snprintf(err, errlen, "aggregator %d: negative domain length %lld", a, (long long)dom_bytes[a]);
            return XG_EARG;
        }
    for (i = 0; i < n; ++i) {
        const xg_ext *e = &exts[i];
        if (e->rank < 0 || e->rank >= procs) {
            snprintf(err, errlen, "extent %lld: rank %d out of range (0..%d)", (long long)i, e->rank, procs - 1);
            return XG_EARG;
        }
        if (e->agg < 0 || e->agg >= cb_nodes) {
            snprintf(err, errlen, "extent %lld: aggregator %d out of range (0..%d)", (long long)i, e->agg,
                     cb_nodes - 1);
            return XG_EARG;
        }
        if (e->off < 0 || e->len < 0) {
            snprintf(err, errlen, "extent %lld: negative offset or length (%lld, %lld)", (long long)i,
                     (long long)e->off, (long long)e->len);
            return XG_EARG;
        }
        if (e->off > INT64_MAX - e->len) {
            snprintf(err, errlen, "extent %lld: offset + length overflow (%lld + %lld)", (long long)i,
                     (long long)e->off, (long long)e->len);
            return XG_EARG;
        }
        if (e->off + e->len > dom_bytes[e->agg]) {
            snprintf(err, errlen, "extent %lld: [%lld, %lld) runs past the domain end of aggregator %d (%lld bytes)",
                     (long long)i, (long long)e->off, (long long)(e->off + e->len), e->agg,
                     (long long)dom_bytes[e->agg]);
            return XG_EARG;
        }
    }
    {   /* a pair's length is the sum of its extents' */
        int64_t *lens = (int64_t *)malloc(sizeof(int64_t) * (size_t)procs * (size_t)cb_nodes);
        if (!lens) {
            snprintf(err, errlen, "extent list: out of host memory");
            return XG_ENOMEM;
        }
        rc = xg_exts_lens(exts, n, procs, cb_nodes, lens);
        free(lens);
        if (rc) {
            snprintf(err, errlen, "extent list: the lengths of one (rank, aggregator) pair overflow");
            return rc;
        }
    }
    if (!scatter || !n) return XG_OK;
    /* two writers to one byte: per aggregator, the positive extents sorted by offset -- each must
     * start at or after the end of the one before (a counting sort by aggregator, then qsort) */
    cnt = (int64_t *)calloc((size_t)cb_nodes + 1, sizeof *cnt);
    beg = (int64_t *)calloc((size_t)cb_nodes + 1, sizeof *beg);
    sp = (span_t *)malloc(sizeof *sp * (size_t)(n + 1));
    if (!cnt || !beg || !sp) {
        snprintf(err, errlen, "extent list: out of host memory");
        rc = XG_ENOMEM;
        goto out;
    }
    for (i = 0; i < n; ++i) cnt[exts[i].agg] += exts[i].len > 0;
    for (a = 0; a < cb_nodes; ++a) beg[a + 1] = beg[a] + cnt[a];
    memset(cnt, 0, sizeof *cnt * ((size_t)cb_nodes + 1));
    for (i = 0; i < n; ++i) {
        span_t *q;
        if (exts[i].len <= 0) continue;
        q = &sp[beg[exts[i].agg] + cnt[exts[i].agg]++];
        q->lo = exts[i].off; q->hi = exts[i].off + exts[i].len; q->at = i;
    }
    for (a = 0; a < cb_nodes && rc == XG_OK; ++a) {
        span_t *v = sp + beg[a];
        const int64_t m = cnt[a];
        qsort(v, (size_t)m, sizeof *v, span_cmp);
        for (i = 1; i < m; ++i)
            if (v[i].lo < v[i - 1].hi) {
                snprintf(err, errlen, "extents %lld and %lld overlap in the domain of aggregator %d ([%lld, %lld) and "
                         "[%lld, %lld)): two writers to one byte", (long long)v[i - 1].at, (long long)v[i].at, a,
                         (long long)v[i - 1].lo, (long long)v[i - 1].hi, (long long)v[i].lo, (long long)v[i].hi);
                rc = XG_EARG;
                break;
            }
    }
out:
    free(cnt); free(beg); free(sp);
    return rc;
}

/* aggregator indices hosted by GPU g precede `a` in its domain buffer when their rank is lower (the
 * order of the aggregator parts of RECV / SEND: rank-major; equal ranks: by index) */
static int dom_before(const xg_sched *s, int b, int a)
{
    return s->rank_list[b] < s->rank_list[a] || (s->rank_list[b] == s->rank_list[a] && b < a);
}

int64_t xg_domain_offset(const xg_sched *s, int ngpus, int a, const int64_t *dom_bytes)
{
    int b, g;
    int64_t o = 0;
    if (!s || !dom_bytes || ngpus <= 0 || a < 0 || a >= s->A) return -1;
    g = xg_gpu_of(s->P, ngpus, s->rank_list[a]);
    for (b = 0; b < s->A; ++b)
        if (b != a && xg_gpu_of(s->P, ngpus, s->rank_list[b]) == g && dom_before(s, b, a)) o += dom_bytes[b];
    return o;
}

int64_t xg_domain_bytes(const xg_sched *s, int ngpus, int g, const int64_t *dom_bytes)
{
    int b;
    int64_t t = 0;
    if (!s || !dom_bytes || ngpus <= 0 || g < 0 || g >= ngpus) return -1;
    for (b = 0; b < s->A; ++b)
        if (xg_gpu_of(s->P, ngpus, s->rank_list[b]) == g) t += dom_bytes[b];
    return t;
}

xg_devplan *xg_place_plan_build(const xg_sched *s, int ngpus, int g, const xg_ext *exts, int64_t n,
                                const int64_t *dom_bytes)
{
    const int scatter = s && s->dir == XG_A2M;
    xg_devplan *dp;
    int64_t *done = NULL, *dense = NULL, *dom = NULL, i, k = 0, npos = 0;
    int a, r;
    if (!s || !dom_bytes || ngpus <= 0 || g < 0 || g >= ngpus || n < 0 || (n && !exts)) return NULL;
    for (i = 0; i < n; ++i) {
        if (!pair_ok(&exts[i], s->P, s->A)) return NULL;
        npos += exts[i].len > 0 && xg_gpu_of(s->P, ngpus, s->rank_list[exts[i].agg]) == g;
    }
    if (npos > INT32_MAX - 1) return NULL;
    dp = (xg_devplan *)calloc(1, sizeof *dp);
    if (!dp) return NULL;
    dp->copies = (xg_copy *)malloc(sizeof(xg_copy) * (size_t)(npos + 1));
    dp->p2p = (xg_p2p *)malloc(sizeof(xg_p2p));
    dp->steps = (xg_stepplan *)calloc(1, sizeof(xg_stepplan));
    done = (int64_t *)calloc((size_t)s->P * s->A, sizeof *done);    /* bytes of the pair's earlier extents */
    dense = (int64_t *)malloc(sizeof *dense * (size_t)s->P * s->A);   /* the pair's place in the dense layout */
    dom = (int64_t *)malloc(sizeof *dom * (size_t)s->A);
    if (!dp->copies || !dp->p2p || !dp->steps || !done || !dense || !dom) {
        free(done); free(dense); free(dom);
        xg_devplan_free(dp);
        return NULL;
    }
    for (a = 0; a < s->A; ++a) {
        const int ar = s->rank_list[a];
        const int here = xg_gpu_of(s->P, ngpus, ar) == g;
        dom[a] = here ? xg_domain_offset(s, ngpus, a, dom_bytes) : -1;
        for (r = 0; r < s->P; ++r)
            dense[(size_t)r * s->A + a] =
                !here ? -1
                : scatter ? xg_recv_offset(s, ngpus, ar) + xg_slot_offset(s, ar, r)
                          : xg_send_offset(s, ngpus, ar) + xg_seg_offset(s, ar, r);
    }
    for (i = 0; i < n; ++i) {
        const xg_ext *e = &exts[i];
        const size_t pr = (size_t)e->rank * s->A + e->agg;
        if (e->len <= 0) continue;
        if (dom[e->agg] >= 0) {
            xg_copy *c = &dp->copies[k++];
            const int64_t d_off = dense[pr] + done[pr], m_off = dom[e->agg] + e->off;
            c->src_buf = XG_BUF_SEND; c->dst_buf = XG_BUF_RECV;
            c->src_off = scatter ? d_off : m_off;
            c->dst_off = scatter ? m_off : d_off;
            c->len = e->len;
            dp->local_bytes += e->len;
        }
        done[pr] += e->len;
    }
    dp->gpu = g; dp->ngpus = ngpus; dp->nsteps = 1;
    dp->flags = XG_DP_RAGGED | XG_DP_EXTENTS;
    dp->ncopy = (int32_t)k; dp->np2p = 0;
    dp->steps[0].pre_count = (int32_t)k;
    dp->steps[0].post_begin = (int32_t)k;
    {
        const int64_t dense_bytes = xg_region_bytes(s, ngpus, g, scatter ? XG_BUF_RECV : XG_BUF_SEND);
        const int64_t dom_total = xg_domain_bytes(s, ngpus, g, dom_bytes);
        dp->region_bytes[XG_BUF_SEND] = scatter ? dense_bytes : dom_total;
        dp->region_bytes[XG_BUF_RECV] = scatter ? dom_total : dense_bytes;
    }
    free(done); free(dense); free(dom);
    return dp;
}
