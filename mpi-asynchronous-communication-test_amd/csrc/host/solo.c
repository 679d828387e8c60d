/*
 * solo.c -- the solo step engine's tables (kernels.h solo_engine_kernel,
 * include/xg_sched.h xg_solo_tables): a hazard-free run of steps cut into
 * 1 KiB pieces, dealt round-robin over R rails (workgroups), and per rail laid
 * out as rows of `waves` pieces (one per wave of the rail's workgroup: 16, or
 * 1 for rails of a single wave) with the step barriers placed between them.
 *
 * A rail closes a step with a workgroup barrier only if it had pieces in it:
 * the barrier sits in front of the rail's next piece -- in that piece's row,
 * counted in the `before` field of that piece and of every later piece of the
 * row, and in the row's barrier count -- and the step it closes is listed in
 * order; a barrier in front of the rail's end is left to the kernel's closing
 * stamp.  Each barrier precedes a distinct piece, so a row holds at most
 * `waves` of them (the 5-bit `before` field).  A rail's table is padded
 * with empty pieces to an even number of chunks of XG_SOLO_K rows plus one
 * spare chunk (the kernel's double-buffered loop loads one chunk past the
 * last without a branch); the kernel stops after the rows that hold real
 * pieces (meta's last R entries), so the padding costs a table slot, not time.
 *
 * Granule G (16, 4 or 1 bytes): the unit of the offsets and lengths, i.e. the
 * alignment every transfer must have -- 16 for the 16-B loads/stores of aligned
 * segments, 4 and 1 for segment sizes that are not multiples of 16 (any -d); the
 * kernel then moves a piece with 4-B or 1-B accesses (xg_solo_tables_g).
 *
 * One-wave rails (waves = 1) use the WIDE form: a row is one piece, so the row's
 * barrier word carries the piece's length (bits 8-19) beside the barrier count
 * (bits 0-7, all of which precede the piece), and the descriptor is two 32-bit
 * offsets in granules (src | dst << 32): 4-64 GiB windows instead of 16-256 MiB.
 */
#include <stdlib.h>
#include <string.h>

#include "xg.h"
#include "xg_sched.h"

static uint64_t desc(uint64_t src, uint64_t dst, uint64_t len) { return src | (dst << 24) | (len << 48); }

int xg_solo_tables(const xg_span *xfer, const int *step_begin, int nsteps, int rails_max, int waves,
                   uint64_t src_base, uint64_t dst_base, xg_solo_shape *shape, uint64_t *descs, int *meta)
{
    return xg_solo_tables_g(xfer, step_begin, nsteps, rails_max, waves, 16, src_base, dst_base, shape, descs, meta);
}

int xg_solo_tables_g(const xg_span *xfer, const int *step_begin, int nsteps, int rails_max, int waves, int granule,
                     uint64_t src_base, uint64_t dst_base, xg_solo_shape *shape, uint64_t *descs, int *meta)
{
    if (!xfer || !step_begin || !shape || nsteps < 1 || nsteps > XG_SOLO_MAX_STEPS || rails_max < 1 ||
        rails_max > XG_SOLO_MAX_RAILS || (waves != 1 && waves != XG_SOLO_WAVES) ||
        (granule != 16 && granule != 4 && granule != 1) || (granule != 16 && waves != 1))
        return XG_EARG;
    const int nx = step_begin[nsteps];
    const int W = waves;       /* pieces per row: one per wave of a rail */
    const uint64_t G = (uint64_t)granule;
    const int bshift = XG_SOLO_BEFORE_SHIFT(granule);
    const int wide = W == 1;
    const uint64_t offmax = wide ? XG_SOLO_WIDE_OFF_MAX : XG_SOLO_OFF_MAX;
    int64_t total = 0;
    for (int i = 0; i < nx; ++i) {
        const xg_span *x = &xfer[i];
        if ((x->src | x->dst | x->len) & (G - 1)) return XG_EARG;
        if (x->len && (x->src < src_base || x->dst < dst_base || (x->src + x->len - src_base) / G > offmax ||
                       (x->dst + x->len - dst_base) / G > offmax))
            return XG_EARG;
        total += (int64_t)((x->len + XG_SOLO_PIECE - 1) / XG_SOLO_PIECE);
    }
    int64_t r = total / W;
    if (r > rails_max) r = rails_max;
    if (r < 1) r = 1;
    const int rails = (int)r;
    const int64_t chunk = (int64_t)W * XG_SOLO_K;
    const int64_t longest = (total + rails - 1) / rails;     /* round-robin: counts differ by <= 1 */
    const int64_t np = ((longest + 2 * chunk - 1) / (2 * chunk) * 2 + 1) * chunk;
    shape->rails = rails;
    shape->npieces = (int)(np > XG_SOLO_MAX_PIECES ? XG_SOLO_MAX_PIECES + 1 : np);
    shape->nrows = (int)(np / W);
    shape->nmeta = rails * (shape->nrows + 1) + rails * nsteps + rails;
    if (np > XG_SOLO_MAX_PIECES) return XG_EARG;
    if (!descs || !meta) return XG_OK;

    const int nrows = shape->nrows;
    memset(descs, 0, sizeof(uint64_t) * (size_t)rails * np);
    int *close = meta, *cstep = meta + (size_t)rails * (nrows + 1);
    memset(close, 0, sizeof(int) * (size_t)rails * (nrows + 1));
    for (int64_t i = 0; i < (int64_t)rails * nsteps; ++i) cstep[i] = -1;
    int64_t *cnt = calloc((size_t)rails, sizeof(int64_t));    /* pieces dealt to each rail */
    int *nb = calloc((size_t)rails, sizeof(int));              /* barriers placed on each rail */
    char *used = calloc((size_t)rails, 1);
    int64_t *pend = calloc((size_t)rails, sizeof(int64_t));    /* open barrier position per rail, -1 none */
    int *pstep = calloc((size_t)rails, sizeof(int));
    if (!cnt || !nb || !used || !pend || !pstep) {
        free(cnt); free(nb); free(used); free(pend); free(pstep);
        return XG_ENOMEM;
    }
    for (int q = 0; q < rails; ++q) pend[q] = -1;
    int cur = 0;
    for (int t = 0; t < nsteps; ++t) {
        memset(used, 0, (size_t)rails);
        for (int i = step_begin[t]; i < step_begin[t + 1]; ++i)
            for (uint64_t o = 0; o < xfer[i].len; o += XG_SOLO_PIECE) {
                const uint64_t len = xfer[i].len - o < XG_SOLO_PIECE ? xfer[i].len - o : XG_SOLO_PIECE;
                /* a barrier still open on this rail goes in front of this piece */
                if (pend[cur] >= 0) {
                    const int64_t at = pend[cur], row = at / W;
                    close[(size_t)cur * (nrows + 1) + row]++;
                    cstep[(size_t)cur * nsteps + nb[cur]++] = pstep[cur];
                    if (!wide)                                   /* wide: `before` = the row's count */
                        for (int64_t w = at % W; w < W; ++w)
                            descs[(size_t)cur * np + row * W + w] += 1ull << bshift;
                    pend[cur] = -1;
                }
                if (wide) {
                    close[(size_t)cur * (nrows + 1) + cnt[cur]] |= (int)((len / G) << 8);
                    descs[(size_t)cur * np + cnt[cur]++] =
                        ((xfer[i].src + o - src_base) / G) | (((xfer[i].dst + o - dst_base) / G) << 32);
                } else {
                    descs[(size_t)cur * np + cnt[cur]++] +=     /* its `before` bits may be set already */
                        desc((xfer[i].src + o - src_base) / G, (xfer[i].dst + o - dst_base) / G, len / G);
                }
                used[cur] = 1;
                cur = (cur + 1) % rails;
            }
        for (int q = 0; q < rails; ++q)
            if (used[q]) {
                pend[q] = cnt[q];
                pstep[q] = t;
            }
    }
    int *rows = cstep + (size_t)rails * nsteps;               /* rows holding real pieces */
    for (int q = 0; q < rails; ++q) rows[q] = (int)((cnt[q] + W - 1) / W);
    free(cnt); free(nb); free(used); free(pend); free(pstep);
    return XG_OK;
}

/* Step times of a solo segment from its rails' stamps (kernels.h solo_engine_kernel):
 * rail r's stamp of step t is stamps[r * stride + t], 0 where the rail closed nothing;
 * a rail with nothing in step t is done with it when it closed its previous step, so
 * its value for t is its latest nonzero stamp at or before t; step t is over when every
 * rail is: out[t] = max over rails, for t in [s0, s1). */
void xg_solo_reduce_stamps(const uint64_t *stamps, int rails, int64_t stride, int s0, int s1, uint64_t *out)
{
    for (int t = s0; t < s1; ++t) out[t] = 0;
    for (int r = 0; r < rails; ++r) {
        uint64_t carry = 0;
        for (int t = s0; t < s1; ++t) {
            const uint64_t x = stamps[(int64_t)r * stride + t];
            if (x > carry) carry = x;
            if (carry > out[t]) out[t] = carry;
        }
    }
}

/* Each rail's last step with pieces, by the deal of xg_solo_tables_g (every piece of every step
 * in order, round-robin over the rails); -1 for a rail without pieces. */
int xg_solo_rail_last(const xg_span *xfer, const int *step_begin, int nsteps, int rails, int32_t *last)
{
    if (!xfer || !step_begin || !last || nsteps < 1 || rails < 1) return XG_EARG;
    for (int q = 0; q < rails; ++q) last[q] = -1;
    int cur = 0;
    for (int t = 0; t < nsteps; ++t)
        for (int i = step_begin[t]; i < step_begin[t + 1]; ++i)
            for (uint64_t o = 0; o < xfer[i].len; o += XG_SOLO_PIECE) {
                last[cur] = t;
                cur = (cur + 1) % rails;
            }
    return XG_OK;
}

/* The kernel writes a rail's closing stamp -- taken when its last piece is delivered -- to every
 * step behind the rail's last barrier.  That barrier closes the last step but one the rail has
 * pieces in, last[r] being the last; in the steps between the two the rail had nothing, and its time for
 * them is its previous stamp, not the end of its last step: zero them (0 = closed nothing, which
 * xg_solo_reduce_stamps carries over).  Otherwise the time of a heavy last step lands on the first
 * step that some rail sat out before it.  cstep: the tables' [rails][n] closed steps (-1 past the
 * last); stamps[r * stride + s0 + t] is rail r's stamp of the segment's step t < n. */
void xg_solo_carry_tail(uint64_t *stamps, int rails, int64_t stride, int s0, int n, const int *cstep,
                        const int32_t *last)
{
    for (int r = 0; r < rails; ++r) {
        int s_end = 0;
        for (int k = 0; k < n && cstep[(int64_t)r * n + k] >= 0; ++k) s_end = cstep[(int64_t)r * n + k] + 1;
        for (int t = s_end; t < last[r] && t < n; ++t) stamps[(int64_t)r * stride + s0 + t] = 0;
    }
}

/* Step times from stamps (xg_sched.h): the one place where marks, chain stamps and engine
 * stamps become step_done[]. */
static double ticks_before(const uint64_t *st, int last, int t, double wall_hz)
{
    return (double)(st[last] - st[t]) / wall_hz;      /* 64-bit difference: wrap-safe */
}

int xg_step_times(int nsteps, const uint64_t *marks, const uint64_t *chain_stamps, const uint64_t *engine_stamps,
                  const int32_t *seg_of, const int32_t *seg_end, const int32_t *chain_end, const uint8_t *need_mark,
                  double wall_hz, double host_total, double *step_done)
{
    if (nsteps == 0) return XG_OK;                      /* a plan without steps (its tables may all be NULL) */
    if (nsteps < 0 || !step_done || !(wall_hz > 0) || (host_total < 0 && (!marks || !seg_of))) return XG_EARG;
    if (host_total >= 0) {
        /* an armed run: one segment over every step, anchored at the host-measured end */
        if (!engine_stamps) return XG_EARG;
        for (int s = 0; s < nsteps; ++s) {
            const double x = host_total - ticks_before(engine_stamps, nsteps - 1, s, wall_hz);
            step_done[s] = s == nsteps - 1 ? host_total : (x > 0 ? x : 0);
        }
        return 0;
    }
    for (int s = 0; s < nsteps;) {
        const int gi = seg_of[s];
        if (chain_stamps && chain_end && chain_end[s]) {
            /* a chain: launch t + 1 stamped step t's completion, a clock kernel the last one's;
             * the mark behind it anchors them all */
            const int ce = chain_end[s];
            if (ce <= s || ce > nsteps) return XG_EARG;
            const double end = (double)(marks[ce] - marks[0]) / wall_hz;
            for (int t = s; t < ce; ++t) {
                const double x = end - ticks_before(chain_stamps, ce - 1, t, wall_hz);
                step_done[t] = t == ce - 1 ? end : (x > 0 ? x : 0);
            }
            s = ce;
            continue;
        }
        const int e = gi >= 0 ? seg_end[gi] : s + 1;
        if (e <= s || e > nsteps || (gi >= 0 && !engine_stamps)) return XG_EARG;
        if (gi < 0 && need_mark && !need_mark[s]) {     /* not marked: the next marked step's time (below) */
            step_done[s] = -1;
            s = e;
            continue;
        }
        const double end = (double)(marks[e] - marks[0]) / wall_hz;
        /* inside a segment: the wall-clock stamps, anchored at the mark after its launch
         * (the last step of a segment is drained, so its stamp is a delivered time) */
        for (int t = s; t < e; ++t) {
            const double x = end - (gi >= 0 ? ticks_before(engine_stamps, e - 1, t, wall_hz) : 0);
            step_done[t] = t == e - 1 ? end : (x > 0 ? x : 0);
        }
        s = e;
    }
    /* an unmarked step is reported as done when the next marked one is: no Timer reads it
     * (xg_sched_timed_steps), and the last step is always marked */
    for (int s = nsteps - 2; s >= 0; --s)
        if (step_done[s] < 0) step_done[s] = step_done[s + 1];
    return 0;
}
