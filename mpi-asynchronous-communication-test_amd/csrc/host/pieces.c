/*
 * pieces.c -- how copy launches are formed (host side of the copy kernels): which kernel kind a
 * launch runs and how it is cut into workgroup pieces (xg_copy_launch_choose), and whether a
 * step's local copies may share a launch with the previous step's unpacks.
 *
 * One workgroup copies one piece.  A launch of w pieces puts ceil(w / CUs) of them on its
 * busiest CU, and the launch lasts about as long as that CU works: pieces x (piece bytes + a
 * fixed per-workgroup start).  xg_piece_size picks, among the launch's default piece size and
 * its halvings down to 4 KiB (a halving still divides power-of-two segment sizes, so no
 * segment gets a ragged tail piece), the one that least loads the busiest CU; ties keep the
 * larger piece.  Reference: the copies MPI does inside Irecv/Issend/Alltoallw for one step
 * (mpi_test.c:1776,1790, :627,912) -- here one launch per step and part.
 */
#include "xg_sched.h"

#include <stdlib.h>
#include <string.h>

int64_t xg_piece_size(const int64_t *lens, int n, int64_t chunk, int cus, int64_t wg_cost)
{
    int64_t best_c = chunk, cand;
    double best = -1;
    int i;
    if (!lens || n <= 0 || chunk <= 0 || cus <= 0) return chunk;
    for (cand = chunk; cand >= 4096 && (cand & 15) == 0; cand /= 2) {
        int64_t w = 0;
        double cost;
        for (i = 0; i < n; ++i)
            if (lens[i] > 0) w += (lens[i] + cand - 1) / cand;
        if (!w) return chunk;
        cost = (double)((w + cus - 1) / cus) * (double)(cand + wg_cost);
        if (best < 0 || cost < best) {
            best = cost;
            best_c = cand;
        }
    }
    return best_c;
}

/* The tiles of one copy_kernel_x dispatch: a workgroup there takes a run of short pieces instead
 * of one piece, so that a 256-B run does not cost a workgroup start.  Greedy in piece order: a
 * tile closes when the next piece would be its (tile_pieces + 1)-th or would take it past
 * tile_bytes; a piece longer than tile_bytes stands alone. */
int xg_extent_tiles(const int64_t *lens, int n, int64_t tile_bytes, int tile_pieces, int32_t *begin)
{
    int i, nt = 0, cnt = 0;
    int64_t bytes = 0;
    if (tile_bytes < 1 || tile_pieces < 1) return -1;
    if (!lens || n <= 0) {
        if (begin) begin[0] = 0;
        return 0;
    }
    for (i = 0; i < n; ++i) {
        const int64_t l = lens[i] > 0 ? lens[i] : 0;
        if (cnt && (cnt >= tile_pieces || bytes + l > tile_bytes)) cnt = 0;
        if (!cnt) {
            if (begin) begin[nt] = i;
            ++nt;
            bytes = 0;
        }
        ++cnt;
        bytes += l;
    }
    if (begin) begin[nt] = n;
    return nt;
}

/* the external definitions of xg_sched.h's inline index functions */
extern inline uint32_t xg_small_ppc(int64_t len, int64_t piece);
extern inline xg_small_at xg_small_index(uint32_t b, uint32_t copies, int64_t len, int64_t piece, uint32_t k);

/* Workgroup b of a small-piece launch (xg_small_index, xg_sched.h), range-checked. */
int xg_small_piece_at(int64_t b, int64_t copies, int64_t len, int64_t piece, int k, int64_t *copy, int64_t *off,
                      int64_t *n)
{
    xg_small_at a;
    if (b < 0 || copies < 1 || len < 1 || piece < 1 || k < 1 || k > (1 << 20)) return -1;
    if (copies * (int64_t)xg_small_ppc(len, piece) > INT32_MAX || (int64_t)k * xg_small_ppc(len, piece) > INT32_MAX ||
        b >= copies * (int64_t)xg_small_ppc(len, piece))
        return -1;
    a = xg_small_index((uint32_t)b, (uint32_t)copies, len, piece, (uint32_t)k);
    if (copy) *copy = a.copy;
    if (off) *off = a.off;
    if (n) *n = a.n;
    return 0;
}

/* ... of the step engines' counter arithmetic */
extern inline uint32_t xg_eng_grid_tickets(uint32_t W, uint32_t nsteps, int armed);
extern inline uint32_t xg_eng_grid_pre_target(uint32_t base, uint32_t W);
extern inline uint32_t xg_eng_grid_target(uint32_t base, uint32_t W, uint32_t s);
extern inline int xg_eng_waiting(uint32_t count, uint32_t target);
extern inline int xg_eng_last(uint32_t ticket, uint32_t target);
extern inline uint32_t xg_eng_solo_lines(uint32_t R);
extern inline uint32_t xg_eng_solo_per_line(uint32_t R, uint32_t line);
extern inline uint32_t xg_eng_solo_arrive_target(uint32_t base, uint32_t R);
extern inline int xg_eng_solo_line_last(uint32_t a, uint32_t base, uint32_t R, uint32_t line);
extern inline int xg_eng_solo_rails_last(uint32_t b, uint32_t base, uint32_t R);

/* The solo engine's words after `armed` armed launches of R rails (xg_sched.h): every launch adds
 * R to arrive, a line's rails to its fin word and the lines to rails, all modulo 2^32. */
void xg_eng_solo_state_after(uint32_t R, uint32_t armed, xg_eng_solo_state *out)
{
    uint32_t l;
    if (!out) return;
    memset(out, 0, sizeof *out);
    if (R < 1) return;
    out->arrive = armed * R;
    out->rails = armed * xg_eng_solo_lines(R);
    out->go = armed;
    for (l = 0; l < xg_eng_solo_lines(R); ++l) out->fin[l] = armed * xg_eng_solo_per_line(R, l);
}

/* ... and of the strided placement's tile arithmetic */
extern inline int64_t xg_vec_bpt(int64_t len, int64_t tile_bytes, int tile_pieces);
extern inline int64_t xg_vec_row_tiles(int64_t len, int64_t count, int64_t tile_bytes, int tile_pieces);
extern inline xg_vec_at xg_vec_piece_at(int64_t src_off, int64_t dst_off, int64_t src_step, int64_t dst_step,
                                           int64_t len, int64_t count, int64_t tile_bytes, int tile_pieces, int64_t t,
                                           int i);

/* Lane i of tile t of a row (xg_vec_piece_at, xg_sched.h), range-checked. */
int xg_vec_piece(const xg_vrow *row, int64_t tile_bytes, int tile_pieces, int64_t t, int i, int64_t *src_off,
                 int64_t *dst_off, int64_t *n)
{
    xg_vec_at p;
    if (!row || tile_bytes < 1 || tile_pieces < 1 || t < 0 || i < 0 || i >= tile_pieces || row->len <= 0 ||
        row->count <= 0 || t >= xg_vec_row_tiles(row->len, row->count, tile_bytes, tile_pieces))
        return -1;
    p = xg_vec_piece_at(row->src_off, row->dst_off, row->src_step, row->dst_step, row->len, row->count, tile_bytes,
                        tile_pieces, t, i);
    if (src_off) *src_off = p.src_off;
    if (dst_off) *dst_off = p.dst_off;
    if (n) *n = p.n;
    return 0;
}

/* The tile prefix sums of a row table: one workgroup per tile, counted in 32 bits. */
int64_t xg_vec_rows_tiles(const xg_vrow *rows, int64_t n, int64_t tile_bytes, int tile_pieces, int32_t *tile0)
{
    int64_t k, tot = 0;
    if (n < 0 || (n && !rows) || tile_bytes < 1 || tile_pieces < 1) return -1;
    for (k = 0; k < n; ++k) {
        const int64_t t = xg_vec_row_tiles(rows[k].len, rows[k].count, tile_bytes, tile_pieces);
        if (tile0) tile0[k] = (int32_t)tot;
        if (t > INT32_MAX - tot) return -1;
        tot += t;
    }
    if (tile0) tile0[n] = (int32_t)tot;
    return tot;
}

/* ... and of a view's */
extern inline int64_t xg_view_jb(int64_t len, int k, int64_t tile_bytes, int tile_pieces);
extern inline int64_t xg_view_tiles(int64_t len, int64_t count, int k, int64_t tile_bytes, int tile_pieces);
extern inline xg_view_at xg_view_piece_at(int64_t len, int64_t count, int k, int64_t jb, int64_t tile_bytes, int64_t t,
                                          int q);

/* Lane q of tile t of the view rows[0 .. k) (xg_view_piece_at, xg_sched.h), range-checked. */
int xg_view_piece(const xg_vrow *rows, int k, int64_t tile_bytes, int tile_pieces, int64_t t, int q, int *row,
                  int64_t *src_off, int64_t *dst_off, int64_t *n)
{
    xg_view_at p;
    const xg_vrow *r;
    int i;
    if (!rows || k < 1 || tile_bytes < 1 || tile_pieces < 1 || k > tile_pieces || t < 0 || q < 0 || q >= tile_pieces ||
        rows->len <= 0 || rows->count <= 0 || (k > 1 && rows->len > tile_bytes / k))
        return -1;
    for (i = 1; i < k; ++i)
        if (rows[i].len != rows->len || rows[i].count != rows->count || rows[i].src_step != rows->src_step ||
            rows[i].dst_step != rows->dst_step)
            return -1;
    if (t >= xg_view_tiles(rows->len, rows->count, k, tile_bytes, tile_pieces)) return -1;
    p = xg_view_piece_at(rows->len, rows->count, k, xg_view_jb(rows->len, k, tile_bytes, tile_pieces), tile_bytes, t, q);
    r = &rows[p.row];
    if (row) *row = p.row;
    if (src_off) *src_off = p.n ? r->src_off + p.block * (r->count > 1 ? r->src_step : 0) + p.off : 0;
    if (dst_off) *dst_off = p.n ? r->dst_off + p.block * (r->count > 1 ? r->dst_step : 0) + p.off : 0;
    if (n) *n = p.n;
    return 0;
}

void xg_launch_facts_add(xg_launch_facts *f, const xg_copy *c)
{
    if (c->len <= 0) return;
    f->bytes += c->len;
    f->npos++;
    f->bits |= (uint64_t)c->src_off | (uint64_t)c->dst_off | (uint64_t)c->len;
    /* a pack's or unpack's staging side is patched per piece by the device scan: never a row */
    if (c->dst_buf == XG_BUF_STAGE_SEND || c->src_buf == XG_BUF_STAGE_RECV ||
        (f->uniform_len && f->uniform_len != c->len))
        f->uniform_len = -1;
    else
        f->uniform_len = c->len;
}

/* Piece KiB of a copy_kernel_w launch of `bytes`: the largest of 8 / 4 / 2 that still gives every
 * CU a 4-wave workgroup (bytes / piece >= 4 x CUs): a 4 MiB launch in 8 KiB pieces is 512 waves =
 * 128 workgroups, half the chip (the local part of a configs[2] step, profiles/r05/share_launches/);
 * in 4 KiB pieces it is 256 workgroups.  Smaller launches take 2 KiB pieces. */
static int wave_kib_for(int64_t bytes, int cus)
{
    int kib;
    for (kib = 8; kib > 2; kib /= 2)
        if (bytes / ((int64_t)kib << 10) >= 4 * (int64_t)cus) return kib;
    return 2;
}

/* The precedence, top to bottom: EXTENT, WAVE (whose pieces a non-temporal run copies as PIECE),
 * SHIFT, PIECE -- and SMALL in place of PIECE only (xg_sched.h says when each applies). */
int xg_copy_launch_choose(const xg_launch_facts *f, const xg_copy_rules *r, xg_copy_choice *out)
{
    int aligned;
    int64_t small, ppc;
    if (!f || !r || !out || f->bytes <= 0 || f->npos <= 0) return -1;
    aligned = (f->bits & 15) == 0;
    out->kind = XG_COPY_PIECE;
    out->nt = f->nt_run != 0;
    out->kib = out->order = 0;
    out->piece = 0;
    if ((f->dp_flags & XG_DP_EXTENTS) && r->extent_copy && r->chunk <= (1 << 24) &&
        f->bytes <= f->npos * r->extent_mean_max) {
        out->kind = XG_COPY_EXTENT;
    } else if (f->cross && f->bytes >= r->wave_min && f->bytes <= r->wave_max && aligned && !f->nt_cut) {
        const int kib = r->wave_kib ? r->wave_kib : wave_kib_for(f->bytes, r->cus);
        out->piece = (int64_t)kib << 10;
        if (!f->nt_run) {       /* else: the cut says plain, the kernel non-temporal -- PIECE over wave-sized pieces */
            out->kind = XG_COPY_WAVE;
            out->kib = kib;
        }
    } else if ((f->dp_flags & XG_DP_RAGGED) && r->ragged_copy && !aligned) {
        out->kind = XG_COPY_SHIFT;
    }
    if (!out->piece) out->piece = xg_piece_size(f->lens, f->nlens, r->chunk, r->cus, r->wg_cost);
    if (out->kind != XG_COPY_PIECE || !f->may_small || !r->small_pieces || !aligned ||
        f->bytes < r->small_piece_min || f->uniform_len <= 0 || r->small_kib < 1)
        return 0;
    small = (int64_t)r->small_kib << 10;
    ppc = (f->uniform_len + small - 1) / small;
    /* xg_small_index works in 32 bits: the launch's workgroups and a group's */
    if (f->npos * ppc > INT32_MAX || r->small_order * ppc > INT32_MAX) return 0;
    out->kind = XG_COPY_SMALL;
    out->kib = r->small_kib;
    out->order = r->small_order;
    out->piece = small;
    return 0;
}

/* [off, end) of region buf */
typedef struct { int64_t lo, hi; } ival;

static int ival_cmp(const void *x, const void *y)
{
    const ival *a = (const ival *)x, *b = (const ival *)y;
    return a->lo < b->lo ? -1 : a->lo > b->lo;
}

/* sorted intervals of one kind (reads or writes) of a set of copies, per region, with running
 * maxima of their ends: "does [a, b) of region buf meet any of them" in O(log n) */
typedef struct {
    ival *v[XG_NBUF];
    int64_t *reach[XG_NBUF];
    int n[XG_NBUF];
} ivset;

static int ivset_build(ivset *t, const xg_copy *c, int n, int dst_side)
{
    int i, k;
    for (k = 0; k < XG_NBUF; ++k) {
        t->n[k] = 0;
        t->v[k] = (ival *)malloc(sizeof(ival) * ((size_t)n + 1));
        t->reach[k] = (int64_t *)malloc(sizeof(int64_t) * ((size_t)n + 1));
        if (!t->v[k] || !t->reach[k]) return -1;
    }
    for (i = 0; i < n; ++i) {
        const int buf = dst_side ? c[i].dst_buf : c[i].src_buf;
        const int64_t off = dst_side ? c[i].dst_off : c[i].src_off;
        if (c[i].len <= 0 || buf < 0 || buf >= XG_NBUF) continue;
        t->v[buf][t->n[buf]].lo = off;
        t->v[buf][t->n[buf]++].hi = off + c[i].len;
    }
    for (k = 0; k < XG_NBUF; ++k) {
        int64_t m = INT64_MIN;
        qsort(t->v[k], t->n[k], sizeof(ival), ival_cmp);
        for (i = 0; i < t->n[k]; ++i) t->reach[k][i] = m = t->v[k][i].hi > m ? t->v[k][i].hi : m;
    }
    return 0;
}

static int ivset_meets(const ivset *t, int buf, int64_t a, int64_t b)
{
    int lo = 0, hi;
    if (buf < 0 || buf >= XG_NBUF) return 0;
    hi = t->n[buf];
    while (lo < hi) {                                  /* intervals starting before b: [0, lo) */
        const int mid = (lo + hi) / 2;
        if (t->v[buf][mid].lo < b) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 && t->reach[buf][lo - 1] > a;
}

static void ivset_free(ivset *t)
{
    int k;
    for (k = 0; k < XG_NBUF; ++k) { free(t->v[k]); free(t->reach[k]); }
}

/* Step s's local copies (after its stage copies, before its packs) against the bytes step
 * s-1's unpacks write: 1 if any of them reads or writes such a byte -- then they cannot share
 * one launch, whose workgroups run in any order (plan_tables.cc fuses them otherwise).
 * Returns -1 for a bad step. */
int xg_step_local_meets_unpacks(const xg_devplan *dp, int s)
{
    const xg_stepplan *pv, *sp;
    ivset w = {{0}, {0}, {0}};
    int i, hit;
    if (!dp || s < 1 || s >= dp->nsteps) return -1;
    pv = &dp->steps[s - 1];
    sp = &dp->steps[s];
    hit = ivset_build(&w, dp->copies + pv->post_begin, pv->post_count, 1) != 0;   /* refuse the fusion when in doubt */
    for (i = sp->stage_count; i < sp->pre_count && !hit; ++i) {
        const xg_copy *c = &dp->copies[sp->pre_begin + i];
        if (c->dst_buf == XG_BUF_STAGE_SEND) break;          /* the packs start */
        if (c->len <= 0) continue;
        hit = ivset_meets(&w, c->src_buf, c->src_off, c->src_off + c->len) ||
              ivset_meets(&w, c->dst_buf, c->dst_off, c->dst_off + c->len);
    }
    ivset_free(&w);
    return hit;
}

/* Step s's packs against the bytes step s-1's unpacks write: 1 if a pack reads such a byte (a
 * forward out of RECV or SCRATCH: a pack's source may lie in any region) or writes one (an
 * unpack into STAGE_SEND; no schedule has one, any xg_devplan may) -- then the packs cannot
 * share a launch with those unpacks either.  Returns -1 for a bad step. */
int xg_step_packs_meet_unpacks(const xg_devplan *dp, int s)
{
    const xg_stepplan *pv, *sp;
    ivset w = {{0}, {0}, {0}};
    int i, hit;
    if (!dp || s < 1 || s >= dp->nsteps) return -1;
    pv = &dp->steps[s - 1];
    sp = &dp->steps[s];
    hit = ivset_build(&w, dp->copies + pv->post_begin, pv->post_count, 1) != 0;   /* refuse the fusion when in doubt */
    for (i = sp->stage_count; i < sp->pre_count && !hit; ++i) {
        const xg_copy *c = &dp->copies[sp->pre_begin + i];
        if (c->dst_buf != XG_BUF_STAGE_SEND || c->len <= 0) continue;   /* a local copy, or empty */
        hit = ivset_meets(&w, c->src_buf, c->src_off, c->src_off + c->len) ||
              ivset_meets(&w, c->dst_buf, c->dst_off, c->dst_off + c->len);
    }
    ivset_free(&w);
    return hit;
}

/* Step s's stage copies (TAM rank-local memcpy's through SCRATCH) against its other pre copies
 * (local gather/scatter, packs): 1 if one of those reads or writes a byte a stage copy writes,
 * or writes a byte a stage copy reads -- then the stage copies need a launch of their own ahead
 * of the others (xg_devplan_build puts them first for that reason); 0 if all may share one
 * launch, whose workgroups run in any order; -1 for a bad step.  At the README configuration
 * m15 / m16's step 3 (14 stage copies into the aggregation buffers beside 434 local copies into
 * the receive slots) shares one launch. */
int xg_step_stage_meets_rest(const xg_devplan *dp, int s)
{
    const xg_stepplan *sp;
    ivset w = {{0}, {0}, {0}}, r = {{0}, {0}, {0}};
    int i, hit = 0;
    if (!dp || s < 0 || s >= dp->nsteps) return -1;
    sp = &dp->steps[s];
    if (sp->stage_count <= 0) return 0;
    if (ivset_build(&w, dp->copies + sp->pre_begin, sp->stage_count, 1) ||
        ivset_build(&r, dp->copies + sp->pre_begin, sp->stage_count, 0)) {
        hit = 1;                                       /* refuse the fusion when in doubt */
        goto done;
    }
    for (i = sp->stage_count; i < sp->pre_count && !hit; ++i) {
        const xg_copy *c = &dp->copies[sp->pre_begin + i];
        if (c->len <= 0) continue;
        hit = ivset_meets(&w, c->src_buf, c->src_off, c->src_off + c->len) ||
              ivset_meets(&w, c->dst_buf, c->dst_off, c->dst_off + c->len) ||
              ivset_meets(&r, c->dst_buf, c->dst_off, c->dst_off + c->len);
    }
done:
    ivset_free(&w);
    ivset_free(&r);
    return hit;
}
