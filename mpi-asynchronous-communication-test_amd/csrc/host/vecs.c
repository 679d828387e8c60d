/*
 * vecs.c -- placement of exchanged segments by STRIDED RUNS (include/xg_sched.h, xg_vec).
 *
 * A regular file view -- each rank's block of a global array, interleaved row by row with the other
 * ranks' blocks (MPI_Type_vector / MPI_Type_create_subarray) -- is a few numbers per (rank,
 * aggregator) pair.  place.c takes its flattened form, one xg_ext per row; here the view itself is
 * the input: it is checked (xg_vecs_check), turned into the exchange's length matrix (xg_vecs_lens)
 * and into one table row per vec (xg_vec_rows_build), from which every block follows by
 * arithmetic.  Nothing here is O(blocks) except xg_vecs_expand, the definition of what a vec list
 * means, and the block walk xg_vecs_check falls back to for clusters that are not a striped view.
 */
#include "sched_int.h"
#include "xg.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static int positive(const xg_vec *v) { return v->len > 0 && v->count > 0; }

/* off + (count - 1) * stride of a positive vec whose stride is looked at only when count > 1;
 * 0 when it fits int64 (then *last holds it) */
static int last_block(const xg_vec *v, int64_t *last)
{
    int64_t span = 0;
    if (v->count > 1 && __builtin_mul_overflow(v->count - 1, v->stride, &span)) return -1;
    return __builtin_add_overflow(v->off, span, last) ? -1 : 0;
}

int64_t xg_vecs_expand(const xg_vec *v, int64_t n, xg_ext *out, int64_t cap)
{
    int64_t i, j, k = 0;
    if (n < 0 || (n && !v)) return -1;
    for (i = 0; i < n; ++i) {
        int64_t last;
        if (v[i].len < 0 || v[i].count < 0 || (v[i].count > 1 && v[i].stride < 0)) return -1;
        if (!positive(&v[i])) continue;
        if (last_block(&v[i], &last) || last > INT64_MAX - v[i].len || v[i].count > INT64_MAX - k) return -1;
        if (out)
            for (j = 0; j < v[i].count && k + j < cap; ++j) {
                xg_ext *e = &out[k + j];
                e->rank = v[i].rank; e->agg = v[i].agg;
                e->off = v[i].off + j * (v[i].count > 1 ? v[i].stride : 0);
                e->len = v[i].len;
            }
        k += v[i].count;
    }
    return k;
}

int xg_vecs_lens(const xg_vec *v, int64_t n, int procs, int cb_nodes, int64_t *lens)
{
    int64_t i;
    if (procs <= 0 || cb_nodes <= 0 || !lens || n < 0 || (n && !v)) return XG_EARG;
    memset(lens, 0, sizeof(int64_t) * (size_t)procs * (size_t)cb_nodes);
    for (i = 0; i < n; ++i) {
        int64_t *l, bytes;
        if (v[i].len < 0 || v[i].count < 0) return XG_EARG;
        if (!positive(&v[i])) continue;
        if (v[i].rank < 0 || v[i].rank >= procs || v[i].agg < 0 || v[i].agg >= cb_nodes) return XG_EARG;
        if (__builtin_mul_overflow(v[i].count, v[i].len, &bytes)) return XG_EARG;
        l = &lens[(size_t)v[i].rank * cb_nodes + v[i].agg];
        if (*l > INT64_MAX - bytes) return XG_EARG;
        *l += bytes;
    }
    return XG_OK;
}

/* ---------------------------------------------------------------- the scatter check */
typedef struct { int64_t lo, hi, at; } hull_t;        /* [lo, hi) of a domain, list index `at` */

static int hull_cmp(const void *x, const void *y)
{
    const hull_t *a = (const hull_t *)x, *b = (const hull_t *)y;
    if (a->lo != b->lo) return a->lo < b->lo ? -1 : 1;
    return a->at < b->at ? -1 : a->at > b->at;
}

/* the heap of a block walk: a vec's next block, keyed by its start (ties: list index) */
typedef struct { int64_t lo, at, j; } blk_t;

static int blk_less(const blk_t *a, const blk_t *b) { return a->lo != b->lo ? a->lo < b->lo : a->at < b->at; }

static void heap_down(blk_t *h, int64_t m, int64_t i)
{
    for (;;) {
        int64_t c = 2 * i + 1;
        blk_t t;
        if (c >= m) return;
        if (c + 1 < m && blk_less(&h[c + 1], &h[c])) ++c;
        if (!blk_less(&h[c], &h[i])) return;
        t = h[i]; h[i] = h[c]; h[c] = t;
        i = c;
    }
}

static void overlap_msg(char *err, size_t errlen, int a, int64_t at0, int64_t j0, int64_t lo0, int64_t hi0, int64_t at1,
                        int64_t j1, int64_t lo1, int64_t hi1)
{
    snprintf(err, errlen, "vec %lld block %lld and vec %lld block %lld overlap in the domain of aggregator %d "
             "([%lld, %lld) and [%lld, %lld)): two writers to one byte", (long long)at0, (long long)j0, (long long)at1,
             (long long)j1, a, (long long)lo0, (long long)hi0, (long long)lo1, (long long)hi1);
}

/* A cluster of vecs whose hulls meet.  The striped view first: every vec with count > 1 and the same
 * stride S, and the intervals [off mod S, off mod S + len) pairwise disjoint on the circle of S --
 * then no block of one meets a block of another, wherever their hulls lie.  h is scratch (m entries). */
static int cluster_striped(const xg_vec *v, const hull_t *c, int64_t m, hull_t *h)
{
    const int64_t S = v[c[0].at].stride;
    int64_t i;
    for (i = 0; i < m; ++i) {
        const xg_vec *q = &v[c[i].at];
        if (q->count <= 1 || q->stride != S) return 0;
        h[i].lo = q->off % S; h[i].hi = h[i].lo + q->len; h[i].at = c[i].at;     /* len <= S: hi < 2 S, no overflow */
        if (h[i].hi < h[i].lo) return 0;
    }
    qsort(h, (size_t)m, sizeof *h, hull_cmp);
    for (i = 1; i < m; ++i)
        if (h[i].lo < h[i - 1].hi) return 0;
    return h[m - 1].hi - S <= h[0].lo;               /* the last one may wrap round to the first */
}

/* ... any other cluster: its blocks in ascending order of their starts, each against the one before
 * (all earlier blocks end at or before that one's end once none overlapped).  0, or 1 with err set. */
static int cluster_walk(const xg_vec *v, const hull_t *c, int64_t m, blk_t *h, int a, char *err, size_t errlen)
{
    int64_t i, left = m, p_at = -1, p_j = 0, p_lo = 0, p_hi = INT64_MIN;
    for (i = 0; i < m; ++i) { h[i].lo = v[c[i].at].off; h[i].at = c[i].at; h[i].j = 0; }
    for (i = m / 2 - 1; i >= 0; --i) heap_down(h, m, i);
    while (left > 0) {
        const xg_vec *q = &v[h[0].at];
        const int64_t lo = h[0].lo, hi = lo + q->len;
        if (lo < p_hi) {
            overlap_msg(err, errlen, a, p_at, p_j, p_lo, p_hi, h[0].at, h[0].j, lo, hi);
            return 1;
        }
        p_at = h[0].at; p_j = h[0].j; p_lo = lo; p_hi = hi;
        if (h[0].j + 1 < q->count) {
            h[0].j++;
            h[0].lo += q->stride;
        } else {
            h[0] = h[--left];
        }
        heap_down(h, left, 0);
    }
    return 0;
}

int xg_vecs_check(const xg_vec *v, int64_t n, int procs, int cb_nodes, const int64_t *dom_bytes, int scatter,
                  char *err, size_t errlen)
{
    char ebuf[8];
    int64_t i, *cnt = NULL, *beg = NULL;
    hull_t *sp = NULL, *tmp = NULL;
    blk_t *heap = NULL;
    int a, rc = XG_OK;
    if (!err) { err = ebuf; errlen = sizeof ebuf; }
    if (errlen) err[0] = 0;
    if (procs <= 0 || cb_nodes <= 0 || n < 0 || (n && !v) || !dom_bytes) {
        snprintf(err, errlen, "vec list: bad arguments (procs %d, cb_nodes %d, n %lld)", procs, cb_nodes, (long long)n);
        return XG_EARG;
    }
    for (a = 0; a < cb_nodes; ++a)
        if (dom_bytes[a] < 0) {
            snprintf(err, errlen, "aggregator %d: negative domain length %lld", a, (long long)dom_bytes[a]);
            return XG_EARG;
        }
    for (i = 0; i < n; ++i) {
        const xg_vec *e = &v[i];
        int64_t last;
        if (e->len < 0 || e->count < 0 || (e->count > 1 && e->stride < 0)) {
            snprintf(err, errlen, "vec %lld: negative length, count or stride (%lld, %lld, %lld)", (long long)i,
                     (long long)e->len, (long long)e->count, (long long)e->stride);
            return XG_EARG;
        }
        if (!positive(e)) continue;
        if (e->rank < 0 || e->rank >= procs) {
            snprintf(err, errlen, "vec %lld: rank %d out of range (0..%d)", (long long)i, e->rank, procs - 1);
            return XG_EARG;
        }
        if (e->agg < 0 || e->agg >= cb_nodes) {
            snprintf(err, errlen, "vec %lld: aggregator %d out of range (0..%d)", (long long)i, e->agg, cb_nodes - 1);
            return XG_EARG;
        }
        if (e->off < 0) {
            snprintf(err, errlen, "vec %lld: negative offset %lld", (long long)i, (long long)e->off);
            return XG_EARG;
        }
        if (last_block(e, &last) || last > INT64_MAX - e->len) {
            snprintf(err, errlen, "vec %lld: offset + (count - 1) * stride + length overflow (%lld + %lld * %lld + %lld)",
                     (long long)i, (long long)e->off, (long long)(e->count - 1), (long long)e->stride,
                     (long long)e->len);
            return XG_EARG;
        }
        if (last + e->len > dom_bytes[e->agg]) {     /* the last block ends last: stride >= 0 */
            snprintf(err, errlen, "vec %lld: its last block [%lld, %lld) runs past the domain end of aggregator %d "
                     "(%lld bytes)", (long long)i, (long long)last, (long long)(last + e->len), e->agg,
                     (long long)dom_bytes[e->agg]);
            return XG_EARG;
        }
    }
    {   /* a pair's length is the sum of its blocks' */
        int64_t *lens = (int64_t *)malloc(sizeof(int64_t) * (size_t)procs * (size_t)cb_nodes);
        if (!lens) {
            snprintf(err, errlen, "vec list: out of host memory");
            return XG_ENOMEM;
        }
        rc = xg_vecs_lens(v, n, procs, cb_nodes, lens);
        free(lens);
        if (rc) {
            snprintf(err, errlen, "vec list: the lengths of one (rank, aggregator) pair overflow");
            return rc;
        }
    }
    if (!scatter || !n) return XG_OK;
    /* two writers to one byte.  Inside a vec: blocks closer than they are long. */
    for (i = 0; i < n; ++i)
        if (positive(&v[i]) && v[i].count > 1 && v[i].stride < v[i].len) {
            overlap_msg(err, errlen, v[i].agg, i, 0, v[i].off, v[i].off + v[i].len, i, 1, v[i].off + v[i].stride,
                        v[i].off + v[i].stride + v[i].len);
            return XG_EARG;
        }
    /* Between vecs: per aggregator (a counting sort), the hulls sorted by their starts and swept into
     * clusters of hulls that meet */
    cnt = (int64_t *)calloc((size_t)cb_nodes + 1, sizeof *cnt);
    beg = (int64_t *)calloc((size_t)cb_nodes + 1, sizeof *beg);
    sp = (hull_t *)malloc(sizeof *sp * (size_t)(n + 1));
    tmp = (hull_t *)malloc(sizeof *tmp * (size_t)(n + 1));
    heap = (blk_t *)malloc(sizeof *heap * (size_t)(n + 1));
    if (!cnt || !beg || !sp || !tmp || !heap) {
        snprintf(err, errlen, "vec list: out of host memory");
        rc = XG_ENOMEM;
        goto out;
    }
    for (i = 0; i < n; ++i)
        if (positive(&v[i])) cnt[v[i].agg]++;
    for (a = 0; a < cb_nodes; ++a) beg[a + 1] = beg[a] + cnt[a];
    memset(cnt, 0, sizeof *cnt * ((size_t)cb_nodes + 1));
    for (i = 0; i < n; ++i) {
        hull_t *q;
        int64_t last = 0;
        if (!positive(&v[i])) continue;
        q = &sp[beg[v[i].agg] + cnt[v[i].agg]++];
        (void)last_block(&v[i], &last);
        q->lo = v[i].off; q->hi = last + v[i].len; q->at = i;
    }
    for (a = 0; a < cb_nodes && rc == XG_OK; ++a) {
        hull_t *h = sp + beg[a];
        const int64_t m = cnt[a];
        int64_t c0 = 0;
        qsort(h, (size_t)m, sizeof *h, hull_cmp);
        while (c0 < m && rc == XG_OK) {
            int64_t c1 = c0 + 1, reach = h[c0].hi;
            while (c1 < m && h[c1].lo < reach) {
                if (h[c1].hi > reach) reach = h[c1].hi;
                ++c1;
            }
            if (c1 - c0 > 1 && !cluster_striped(v, h + c0, c1 - c0, tmp) &&
                cluster_walk(v, h + c0, c1 - c0, heap, a, err, errlen))
                rc = XG_EARG;
            c0 = c1;
        }
    }
out:
    free(cnt); free(beg); free(sp); free(tmp); free(heap);
    return rc;
}

/* ---------------------------------------------------------------- rows */
int64_t xg_vec_rows_build(const xg_sched *s, int ngpus, int g, const xg_vec *v, int64_t n, const int64_t *dom_bytes,
                          xg_vrow *rows, int64_t *vec_index, int64_t *region_bytes)
{
    const int scatter = s && s->dir == XG_A2M;
    int64_t *done = NULL, *dense = NULL, *dom = NULL, i, k = 0;
    int a, r;
    if (!s || !dom_bytes || ngpus <= 0 || g < 0 || g >= ngpus || n < 0 || (n && !v)) return -1;
    for (i = 0; i < n; ++i)
        if (positive(&v[i]) && (v[i].rank < 0 || v[i].rank >= s->P || v[i].agg < 0 || v[i].agg >= s->A)) return -1;
    if (region_bytes) {
        const int64_t dense_bytes = xg_region_bytes(s, ngpus, g, scatter ? XG_BUF_RECV : XG_BUF_SEND);
        const int64_t dom_total = xg_domain_bytes(s, ngpus, g, dom_bytes);
        memset(region_bytes, 0, sizeof(int64_t) * XG_NBUF);
        region_bytes[XG_BUF_SEND] = scatter ? dense_bytes : dom_total;
        region_bytes[XG_BUF_RECV] = scatter ? dom_total : dense_bytes;
    }
    done = (int64_t *)calloc((size_t)s->P * s->A, sizeof *done);      /* bytes of the pair's earlier vecs */
    dense = (int64_t *)malloc(sizeof *dense * (size_t)s->P * s->A);     /* the pair's place in the dense layout */
    dom = (int64_t *)malloc(sizeof *dom * (size_t)s->A);
    if (!done || !dense || !dom) {
        free(done); free(dense); free(dom);
        return -1;
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
        const xg_vec *e = &v[i];
        const size_t pr = (size_t)e->rank * s->A + e->agg;
        if (!positive(e)) continue;
        if (dom[e->agg] >= 0) {
            if (rows) {
                xg_vrow *w = &rows[k];
                const int64_t d_off = dense[pr] + done[pr], m_off = dom[e->agg] + e->off;
                const int64_t d_step = e->count > 1 ? e->len : 0, m_step = e->count > 1 ? e->stride : 0;
                w->src_buf = XG_BUF_SEND; w->dst_buf = XG_BUF_RECV;
                w->src_off = scatter ? d_off : m_off;
                w->dst_off = scatter ? m_off : d_off;
                w->src_step = scatter ? d_step : m_step;
                w->dst_step = scatter ? m_step : d_step;
                w->len = e->len; w->count = e->count;
            }
            if (vec_index) vec_index[k] = i;
            ++k;
        }
        done[pr] += e->count * e->len;
    }
    free(done); free(dense); free(dom);
    return k;
}

/* ------------------------------------------------------------------ views
 * Which rows of a GPU's row list are one striped file view (xg_vrow_views, xg_sched.h): the
 * recognition copy_kernel_vv's tables (vec_tables.cc, xg_view_tables_build) are built from.  The most
 * common MPI-IO view is a domain striped over the ranks in runs of L bytes: rank r's row holds block
 * j at r x L + j x P x L of the domain, so the rows of the P ranks are L apart on the domain side and
 * equal in everything else.  A rank-major vec list puts them cb_nodes apart in the row list, so they
 * are found by sorting, never by looking at neighbours. */
typedef struct { const xg_vrow *r; int64_t idx; } vent;

static int cmp64(int64_t a, int64_t b) { return a < b ? -1 : a > b; }

/* everything the rows of a view share; 0 when equal */
static int cmp_shape(const xg_vrow *a, const xg_vrow *b)
{
    int c;
    if ((c = cmp64(a->src_buf, b->src_buf)) || (c = cmp64(a->dst_buf, b->dst_buf)) || (c = cmp64(a->len, b->len)) ||
        (c = cmp64(a->count, b->count)) || (c = cmp64(a->src_step, b->src_step)))
        return c;
    return cmp64(a->dst_step, b->dst_step);
}

/* total orders: the shape, the striped offset, the other offset, the list index */
static int cmp_dst(const void *x, const void *y)
{
    const vent *a = (const vent *)x, *b = (const vent *)y;
    int c;
    if ((c = cmp_shape(a->r, b->r)) || (c = cmp64(a->r->dst_off, b->r->dst_off)) ||
        (c = cmp64(a->r->src_off, b->r->src_off)))
        return c;
    return cmp64(a->idx, b->idx);
}

static int cmp_src(const void *x, const void *y)
{
    const vent *a = (const vent *)x, *b = (const vent *)y;
    int c;
    if ((c = cmp_shape(a->r, b->r)) || (c = cmp64(a->r->src_off, b->r->src_off)) ||
        (c = cmp64(a->r->dst_off, b->r->dst_off)))
        return c;
    return cmp64(a->idx, b->idx);
}

/* may this row be one of several of a view */
static int chains(const xg_vrow *r, int64_t tile_bytes) { return r->len > 0 && r->count > 0 && r->len <= tile_bytes; }

/* b follows a in a chain: the same shape, the striped offset len on (an offset that wraps never chains) */
static int follows(const xg_vrow *a, const xg_vrow *b, int src_side)
{
    const int64_t ao = src_side ? a->src_off : a->dst_off, bo = src_side ? b->src_off : b->dst_off;
    return cmp_shape(a, b) == 0 && ao <= INT64_MAX - a->len && bo == ao + a->len;
}

/* One view per entry of `first`: its chain's start in the sorted array it was found in.  Views of the
 * second pass are merged into the first pass's order by their first row's position there (pos1). */
typedef struct { int64_t pos1, idx; int64_t at, k; int32_t kind; } view;

static int cmp_view(const void *x, const void *y)
{
    const view *a = (const view *)x, *b = (const view *)y;
    int c = cmp64(a->pos1, b->pos1);
    return c ? c : cmp64(a->idx, b->idx);
}

int64_t xg_vrow_views(const xg_vrow *rows, int64_t n, int64_t tile_bytes, int tile_pieces, int64_t *order,
                      int32_t *view_k, int32_t *view_kind)
{
    vent *a = NULL, *b = NULL;          /* the first sort; the rows it left single, sorted again */
    int64_t *pos1 = NULL;               /* a row's position in the first sort */
    view *v = NULL;
    int64_t i, e, m = 0, nv = 0, out = 0;
    if (n < 0 || (n && !rows) || tile_bytes < 1 || tile_pieces < 1) return -1;
    if (n == 0) return 0;
    a = (vent *)malloc(sizeof *a * (size_t)n);
    b = (vent *)malloc(sizeof *b * (size_t)n);
    pos1 = (int64_t *)malloc(sizeof *pos1 * (size_t)n);
    v = (view *)malloc(sizeof *v * (size_t)n);
    if (!a || !b || !pos1 || !v) {
        free(a); free(b); free(pos1); free(v);
        return -1;
    }
    for (i = 0; i < n; ++i) { a[i].r = &rows[i]; a[i].idx = i; }
    qsort(a, (size_t)n, sizeof *a, cmp_dst);
    for (i = 0; i < n; ++i) pos1[a[i].idx] = i;
    /* pass 1: chains by destination offset; [i, e) is one */
    for (i = 0; i < n; i = e) {
        e = i + 1;
        if (chains(a[i].r, tile_bytes))
            while (e < n && follows(a[e - 1].r, a[e].r, 0)) ++e;
        if (e - i == 1) {
            b[m++] = a[i];
            continue;
        }
        v[nv].pos1 = i; v[nv].idx = a[i].idx; v[nv].at = i; v[nv].k = e - i; v[nv].kind = XG_VIEW_DST_STRIPED;
        ++nv;
    }
    /* pass 2: what is left, by source offset; at < 0 marks a view whose rows are b's */
    qsort(b, (size_t)m, sizeof *b, cmp_src);
    for (i = 0; i < m; i = e) {
        e = i + 1;
        if (chains(b[i].r, tile_bytes))
            while (e < m && follows(b[e - 1].r, b[e].r, 1)) ++e;
        v[nv].pos1 = pos1[b[i].idx]; v[nv].idx = b[i].idx; v[nv].at = -1 - i; v[nv].k = e - i;
        v[nv].kind = e - i > 1 ? XG_VIEW_SRC_STRIPED : XG_VIEW_SINGLE;
        ++nv;
    }
    qsort(v, (size_t)nv, sizeof *v, cmp_view);
    /* the views in order, a chain longer than kmax in consecutive views of kmax rows */
    for (i = 0, e = 0; i < nv; ++i) {
        const vent *from = v[i].at >= 0 ? a + v[i].at : b + (-1 - v[i].at);
        int64_t kmax = 1, done, j;
        if (v[i].k > 1) {
            kmax = tile_bytes / from->r->len;
            if (kmax > tile_pieces) kmax = tile_pieces;
            if (kmax < 1) kmax = 1;
        }
        for (done = 0; done < v[i].k; done += kmax) {
            const int64_t k = v[i].k - done < kmax ? v[i].k - done : kmax;
            if (order)
                for (j = 0; j < k; ++j) order[e + j] = from[done + j].idx;
            e += k;
            if (view_k) view_k[out] = (int32_t)k;
            if (view_kind) view_kind[out] = k > 1 ? v[i].kind : XG_VIEW_SINGLE;
            ++out;
        }
    }
    free(a); free(b); free(pos1); free(v);
    return out;
}
