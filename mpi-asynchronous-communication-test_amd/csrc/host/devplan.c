/*
 * devplan.c -- the per-GPU device plan of a compiled schedule (xg_devplan_build_form): per step,
 * the GPU's local copies, packs into per-peer staging, its RCCL calls in the direct, packed
 * one-sided / two-sided or relay form, and unpacks.  The builder holds its state in one context
 * (bcx), indexes each step's messages by GPU pair once (step_index) and runs the step as named parts
 * (step_*); a peer's sends and receives come from one body per form, given a direction.  Plain C99,
 * no HIP.  See include/xg_sched.h; the calls each step posts and their pairing proof are calls.c.
 */
#include "sched_int.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ device plan */
/* Growable arrays of the device-plan builder.  The builder runs on every rank of a job and
 * must not stop one rank alone: when the host runs out of memory, a push lands in `sink` and
 * `fail` is set; xg_devplan_build_form then frees what it built and returns NULL, which the
 * caller turns into an error every rank agrees on (agree.h: agree_peers). */
typedef struct { void *v; size_t esz; int n, cap, fail; union { xg_copy c; xg_p2p p; } sink; } gvec;
static void *gpush(gvec *c)     /* -> a zeroed new element of esz bytes */
{
    if (c->n == c->cap) {
        const int cap = c->cap ? 2 * c->cap : 256;
        void *v = c->fail ? NULL : realloc(c->v, c->esz * cap);
        if (!v) { c->fail = 1; return memset(&c->sink, 0, sizeof c->sink); }
        c->v = v; c->cap = cap;
    }
    return memset((char *)c->v + c->esz * c->n++, 0, c->esz);
}
static xg_copy *cpush(gvec *c) { return (xg_copy *)gpush(c); }
static xg_p2p *ppush(gvec *c) { return (xg_p2p *)gpush(c); }

void xg_devplan_free(xg_devplan *p)
{
    if (!p) return;
    free(p->copies); free(p->p2p); free(p->steps); free(p);
}

/* same decision on both ends of a (step, src gpu, dst gpu) transfer list: >= 2 segments, mean
 * below pack_max_seg, and at least pack_min bytes (below that one RCCL call per segment costs
 * less than the pack and unpack launches) */
static int use_pack(int n, int64_t total, int64_t pack_max_seg, int64_t pack_min)
{
    return pack_max_seg > 0 && n >= 2 && total / n < pack_max_seg && total >= pack_min;
}

/* region base of every rank hosted by the GPU the plan is for */
typedef struct { int64_t *base[XG_NBUF]; } plan_bases;

/* -> 0, or -1 when the host is out of memory (pb is then freeable) */
static int plan_bases_init(plan_bases *pb, const xg_sched *s, int G)
{
    int lo, hi, r, k, fail = 0;
    int64_t scr = 0;
    for (k = 0; k < XG_NBUF; ++k) fail |= !(pb->base[k] = (int64_t *)calloc(s->P + 1, sizeof(int64_t)));
    if (fail) return -1;
    for (r = 0; r < s->P; ++r) {
        pb->base[XG_BUF_SEND][r] = xg_send_offset(s, G, r);
        pb->base[XG_BUF_RECV][r] = xg_recv_offset(s, G, r);
    }
    for (k = 0; k < G; ++k) {
        xg_block_range(s->P, G, k, &lo, &hi);
        for (scr = 0, r = lo; r < hi; ++r) { pb->base[XG_BUF_SCRATCH][r] = scr; scr += s->scr_size[r]; }
    }
    return 0;
}

static void plan_bases_free(plan_bases *pb)
{
    int k;
    for (k = 0; k < XG_NBUF; ++k) free(pb->base[k]);
}

static int64_t src_off(const plan_bases *pb, const xg_msg *m) { return pb->base[m->sbuf][m->src] + m->soff; }
static int64_t dst_off(const plan_bases *pb, const xg_msg *m) { return pb->base[m->dbuf][m->dst] + m->doff; }

/* a message that moves device bytes (not a size message, not empty) */
static int moves(const xg_msg *m) { return m->len > 0 && !(m->flags & XG_MSG_CTRL); }

/* a rank-local memcpy through a TAM aggregation buffer.  It never crosses GPUs: XG_MSG_COPY is set
 * on the self copies alone, which sched.c's do_match makes with src == dst (one rank, one GPU) */
static int is_stage(const xg_msg *m)
{
    return (m->flags & XG_MSG_COPY) && (m->sbuf == XG_BUF_SCRATCH || m->dbuf == XG_BUF_SCRATCH);
}

xg_devplan *xg_devplan_build(const xg_sched *s, int ngpus, int g, int64_t pack_max_seg)
{
    return xg_devplan_build_form(s, ngpus, g, pack_max_seg, 0, XG_PACK_FORM_DEFAULT);
}

xg_devplan *xg_devplan_build_ex(const xg_sched *s, int ngpus, int g, int64_t pack_max_seg, int64_t pack_min)
{
    return xg_devplan_build_form(s, ngpus, g, pack_max_seg, pack_min, XG_PACK_FORM_DEFAULT);
}

/* One-sided form of one packed (step, src GPU -> dst GPU) transfer list (XG_PACK_ONE_SIDED).
 * The messages are put in destination order (by_src = 0) or source order (by_src = 1) and
 * merged into RUNS, each contiguous on that side: one RCCL call per run.  A run that is
 * contiguous on the other side as well moves straight between the regions; any other one is
 * gathered into staging by the sender (destination order) or scattered out of it by the
 * receiver (source order) -- so every byte is copied on ONE side at most, where the two-sided
 * form packs and unpacks all of them.  This is the transpose the alltoallw datatypes of m5/m8
 * describe (mpi_test.c:233-302): e.g. all-to-many at P64 A16 on 8 GPUs, per peer the 16
 * segments of 8 senders for 2 aggregators -- 2 runs of 2 MiB, one per aggregator's receive
 * slots, gathered on the sending GPU; nothing is unpacked.  Of the two orders the one with
 * fewer copied bytes + XG_RUN_CALL_BYTES per call wins (ties: destination order).  Both GPUs
 * of the pair derive it from the same message list, so their calls pair one to one. */
typedef struct {
    int n, nrun, by_src, fail;   /* fail: out of host memory (the plan is discarded) */
    int *idx;                 /* message indices, run order */
    int *run_b;               /* run r = idx[run_b[r] .. run_b[r + 1]) */
    unsigned char *staged;    /* run r goes through staging */
} oneside;

static const xg_msg *os_msg(const xg_sched *s, const oneside *o, int i) { return &s->msgs[o->idx[i]]; }

typedef struct { int64_t off; int32_t buf, idx; } os_key;
static int os_cmp(const void *a, const void *b)
{
    const os_key *x = (const os_key *)a, *y = (const os_key *)b;
    if (x->buf != y->buf) return x->buf < y->buf ? -1 : 1;
    if (x->off != y->off) return x->off < y->off ? -1 : 1;
    return x->idx < y->idx ? -1 : x->idx > y->idx;      /* equal addresses: message order */
}

/* runs of `o` in the order by_src; returns the cost (copied bytes + calls) */
static int64_t os_layout(const xg_sched *s, const plan_bases *pb, oneside *o, int by_src)
{
    int i, r;
    int64_t cost = 0;
    os_key *key = (os_key *)malloc(sizeof(os_key) * ((size_t)o->n + 1));
    o->by_src = by_src;
    if (!key) {
        o->fail = 1;
        o->nrun = 0;
        return 0;
    }
    for (i = 0; i < o->n; ++i) {
        const xg_msg *m = os_msg(s, o, i);
        key[i].buf = by_src ? m->sbuf : m->dbuf;
        key[i].off = by_src ? src_off(pb, m) : dst_off(pb, m);
        key[i].idx = o->idx[i];
    }
    qsort(key, (size_t)o->n, sizeof(os_key), os_cmp);
    for (i = 0; i < o->n; ++i) o->idx[i] = key[i].idx;
    free(key);
    o->nrun = 0;
    for (i = 0; i < o->n; ++i) {
        const xg_msg *m = os_msg(s, o, i);
        if (i > 0) {
            const xg_msg *q = os_msg(s, o, i - 1);
            const int contiguous = by_src ? (m->sbuf == q->sbuf && src_off(pb, m) == src_off(pb, q) + q->len)
                                          : (m->dbuf == q->dbuf && dst_off(pb, m) == dst_off(pb, q) + q->len);
            if (contiguous) continue;
        }
        o->run_b[o->nrun++] = i;
    }
    o->run_b[o->nrun] = o->n;
    for (r = 0; r < o->nrun; ++r) {
        int64_t bytes = 0;
        int other = 1;      /* contiguous on the other side too */
        for (i = o->run_b[r]; i < o->run_b[r + 1]; ++i) {
            const xg_msg *m = os_msg(s, o, i);
            bytes += m->len;
            if (i > o->run_b[r]) {
                const xg_msg *q = os_msg(s, o, i - 1);
                other &= by_src ? (m->dbuf == q->dbuf && dst_off(pb, m) == dst_off(pb, q) + q->len)
                                : (m->sbuf == q->sbuf && src_off(pb, m) == src_off(pb, q) + q->len);
            }
        }
        o->staged[r] = !other;
        cost += (other ? 0 : bytes) + XG_RUN_CALL_BYTES;
    }
    return cost;
}

/* frees the arrays; keeps `fail` for the caller to see */
static void os_free(oneside *o)
{
    const int fail = o->fail;
    free(o->idx); free(o->run_b); free(o->staged);
    memset(o, 0, sizeof *o);
    o->fail = fail;
}

/* the one-sided form of a step's n messages msgs[] from one GPU to another (a bucket of the index) */
static void os_build(const xg_sched *s, const plan_bases *pb, const int *msgs, int n, oneside *o)
{
    int64_t cost_d, cost_s;
    o->n = n;
    o->idx = (int *)malloc(sizeof(int) * ((size_t)o->n + 1));
    o->run_b = (int *)malloc(sizeof(int) * ((size_t)o->n + 2));
    o->staged = (unsigned char *)malloc((size_t)o->n + 1);
    if (!o->idx || !o->run_b || !o->staged) { os_free(o); o->fail = 1; return; }
    memcpy(o->idx, msgs, sizeof(int) * (size_t)n);
    cost_s = os_layout(s, pb, o, 1);
    cost_d = os_layout(s, pb, o, 0);
    if (cost_s < cost_d) os_layout(s, pb, o, 1);
}

/* ---- the builder's context: all xg_devplan_build_form holds while it builds one GPU's plan.
 * bcx_init allocates it and bcx_free frees it; a failed allocation sets `oom`, and the builder then
 * frees what it has and returns NULL (nothing exits on out-of-memory: see gvec above). */
enum { OUT = 0, IN = 1 };           /* a direction of this GPU's traffic with a peer p: [dir * G + p] */
typedef struct {
    const xg_sched *s;
    xg_devplan *dp;                 /* the plan being built */
    plan_bases pb;
    int G, g, form, oom;
    int64_t pack_max_seg, pack_min;
    int *cnt, *order;               /* messages sorted by step: step st is order[cnt[st] .. cnt[st + 1]) */
    gvec pre, post, pp;             /* copies before the exchange, copies after it, RCCL calls */
    int32_t *posts;                 /* xgi_step_posts_of's answer */
    /* of the step being built: */
    int64_t sbase, rbase, soff;     /* STAGE_SEND / STAGE_RECV fill; STAGE_SEND bytes the send calls took */
    int *bk, *bk_off;               /* the index (step_index) */
    int64_t *vol_b;                 /* per direction and peer: bytes (0: no message; p = g: 0) */
    oneside *os;                    /* per direction and peer: the one-sided layout of a packed list */
    int64_t *rl_ei, *rl_p;          /* relay_step's egress [g] and ingress [G + g] bytes; pair bytes */
    int *rl_w;                      /* a weighted step's shares (weighted_step) */
    /* of the coalesced relay (rc_step): */
    int dry;                        /* only sum the unpacked bytes (the relay area starts behind them) */
    const int *w;                   /* weighted step: [(a * G + b) * G + h] = pair (a, b)'s share via h in
                                       1/XG_WEIGHT_ONE (weighted_step); NULL: relay_cut's uniform pieces */
    const xg_msg **pm; int64_t *po, *pl;    /* pieces of the call being built: message, offset in it, length */
    int64_t *blk;                   /* [a * G + b]: where the block of a's pieces for b that g relays lies */
    int64_t ubase, rlbase, rl;      /* STAGE_RECV: unpack fill, relay area start / fill */
} bcx;

static void *bcx_alloc(bcx *x, size_t n, size_t size)
{
    void *p = calloc(n, size);
    x->oom |= !p;
    return p;
}

static void bcx_init(bcx *x, const xg_sched *s, int G, int g, int64_t pack_max_seg, int64_t pack_min, int form)
{
    const size_t nst = (size_t)s->nsteps, GG = (size_t)G * G;
    size_t widest = 0;
    int i;
    memset(x, 0, sizeof *x);
    if (form != XG_PACK_TWO_SIDED && form != XG_PACK_ONE_SIDED && form != XG_RELAY && form != XG_RELAY_COALESCED)
        form = XG_PACK_FORM_DEFAULT;
    x->s = s; x->G = G; x->g = g; x->form = form; x->pack_min = pack_min;
    x->pack_max_seg = form == XG_RELAY || form == XG_RELAY_COALESCED ? 0 : pack_max_seg;   /* every other step is direct */
    x->pre.esz = x->post.esz = sizeof(xg_copy); x->pp.esz = sizeof(xg_p2p);
    x->oom |= plan_bases_init(&x->pb, s, G) != 0;
    x->cnt = (int *)bcx_alloc(x, nst + 2, sizeof(int));
    x->order = (int *)bcx_alloc(x, (size_t)s->nmsg + 1, sizeof(int));
    if (x->oom) return;
    /* counting sort of messages by step, stable in message order (a step's count two places up, so
     * that filling `order` leaves every cnt[st] at its step's begin) */
    for (i = 0; i < s->nmsg; ++i) x->cnt[s->msgs[i].step + 2]++;
    for (i = 0; i < s->nsteps; ++i) {
        if ((size_t)x->cnt[i + 2] > widest) widest = (size_t)x->cnt[i + 2];
        x->cnt[i + 2] += x->cnt[i + 1];
    }
    for (i = 0; i < s->nmsg; ++i) x->order[x->cnt[s->msgs[i].step + 1]++] = i;
    x->posts = (int32_t *)bcx_alloc(x, nst + 1, sizeof(int32_t));
    x->bk = (int *)bcx_alloc(x, widest + 1, sizeof(int));
    x->bk_off = (int *)bcx_alloc(x, GG + 2, sizeof(int));
    x->vol_b = (int64_t *)bcx_alloc(x, 2 * (size_t)G, sizeof(int64_t));
    x->os = (oneside *)bcx_alloc(x, 2 * (size_t)G, sizeof(oneside));
    x->rl_ei = (int64_t *)bcx_alloc(x, 2 * (size_t)G, sizeof(int64_t));
    x->rl_p = (int64_t *)bcx_alloc(x, GG, sizeof(int64_t));
    x->rl_w = (int *)bcx_alloc(x, GG * G, sizeof(int));
    x->pm = (const xg_msg **)bcx_alloc(x, widest + 1, sizeof(xg_msg *));
    x->po = (int64_t *)bcx_alloc(x, widest + 1, sizeof(int64_t));
    x->pl = (int64_t *)bcx_alloc(x, widest + 1, sizeof(int64_t));
    x->blk = (int64_t *)bcx_alloc(x, GG, sizeof(int64_t));
    x->dp = (xg_devplan *)bcx_alloc(x, 1, sizeof(xg_devplan));
    if (x->dp) x->dp->steps = (xg_stepplan *)bcx_alloc(x, nst + 1, sizeof(xg_stepplan));
}

/* frees all but the plan itself */
static void bcx_free(bcx *x)
{
    free(x->pre.v); free(x->post.v); free(x->pp.v); free(x->cnt); free(x->order); free(x->posts);
    free(x->bk); free(x->bk_off); free(x->vol_b); free(x->os); free(x->rl_ei); free(x->rl_p); free(x->rl_w);
    free((void *)x->pm); free(x->po); free(x->pl); free(x->blk);
    plan_bases_free(&x->pb);
}

static const xg_msg *step_msg(const bcx *x, int k) { return &x->s->msgs[x->order[k]]; }

static void local_copy(bcx *x, const xg_msg *m)
{
    xg_copy *c = cpush(&x->pre);
    c->src_buf = m->sbuf; c->src_off = src_off(&x->pb, m);
    c->dst_buf = m->dbuf; c->dst_off = dst_off(&x->pb, m);
    c->len = m->len; x->dp->local_bytes += m->len;
}

/* The filter, stated once: a moving, non-stage message belongs to the bucket of its (source GPU,
 * destination GPU), source GPU * G + destination GPU; any other message to none (-1). */
static int msg_bucket(const bcx *x, const xg_msg *m)
{
    if (!moves(m) || is_stage(m)) return -1;
    return xg_gpu_of(x->s->P, x->G, m->src) * x->G + xg_gpu_of(x->s->P, x->G, m->dst);
}

/* The index of step [b, e): bucket (a, b') = bk[bk_off[a * G + b'] .. bk_off[a * G + b' + 1]), in
 * message order.  Every walk of "the step's messages from GPU a to GPU b'" goes over a bucket;
 * (g, g) is GPU g's local copies.  (relay_step and relay_calls walk the step in message order
 * across pairs: the relay area is laid out in that order.) */
static void step_index(bcx *x, int b, int e)
{
    int k, c;
    memset(x->bk_off, 0, sizeof(int) * ((size_t)x->G * x->G + 2));
    for (k = b; k < e; ++k)
        if ((c = msg_bucket(x, step_msg(x, k))) >= 0) x->bk_off[c + 2]++;
    for (c = 0; c < x->G * x->G; ++c) x->bk_off[c + 2] += x->bk_off[c + 1];
    for (k = b; k < e; ++k)         /* filling leaves every bk_off[c] at its bucket's begin */
        if ((c = msg_bucket(x, step_msg(x, k))) >= 0) x->bk[x->bk_off[c + 1]++] = x->order[k];
}

static const xg_msg *bk_msg(const bcx *x, int k) { return &x->s->msgs[x->bk[k]]; }

/* the bucket this GPU shares with peer p in direction dir (p = g: its local copies) -> bk[lo .. *hi) */
static int peer_bucket(const bcx *x, int p, int dir, int *hi)
{
    const int c = dir == OUT ? x->g * x->G + p : p * x->G + x->g;
    *hi = x->bk_off[c + 1];
    return x->bk_off[c];
}

/* ---- relay form (XG_RELAY, xg_sched.h): two-phase (Valiant) routing of one step.  Every
 * cross-GPU message is cut into G pieces: pieces 0 and 1 go straight to the destination (one per
 * RCCL group), piece 2 + i through relay GPU R[i].  Then EVERY link (a -> h) carries egress(a) / G
 * in the first group and every link (h -> b) ingress(b) / G in the second, whatever the step's
 * traffic matrix: the step costs (max egress + max ingress) / G of link time instead of its
 * busiest GPU pair's bytes.  A step is relayed when that is at most XG_RELAY_GAIN of the direct
 * cost and every cross-GPU message is >= XG_RELAY_MIN_BYTES (smaller pieces are latency, not
 * bandwidth).  Pairwise m9 / m10 (mpi_test.c:510-597, :421-508; partner rank ^ i, :531-545) at
 * configs[3] put every GPU's 16 MiB round on ONE of its 7 links: 16 -> 4 MiB of link time per
 * round.  Every GPU decides from the same message list, so all agree.  -> 1: relay it; 0: the uniform
 * cut does not pay (rl_p holds the step's GPU-pair bytes); -1: no routing can (nothing to relay) */
static int relay_step(const bcx *x, int b, int e)
{
    const int G = x->G;
    int64_t *const egress = x->rl_ei, *const ingress = x->rl_ei + G, *const pair = x->rl_p;
    int k, g, any = 0;
    int64_t direct = 0, emax = 0, imax = 0;
    if (G < 3) return -1;
    memset(egress, 0, sizeof(int64_t) * 2 * (size_t)G);     /* and ingress */
    memset(pair, 0, sizeof(int64_t) * (size_t)G * G);
    for (k = b; k < e; ++k) {
        const xg_msg *m = step_msg(x, k);
        const int c = msg_bucket(x, m), gs = c / G, gd = c % G;
        if (c < 0 || gs == gd) continue;
        if (m->len < XG_RELAY_MIN_BYTES) return -1;
        egress[gs] += m->len;
        ingress[gd] += m->len;
        pair[(size_t)gs * G + gd] += m->len;
        any = 1;
    }
    if (!any) return -1;
    for (g = 0; g < G * G; ++g) direct = pair[g] > direct ? pair[g] : direct;
    for (g = 0; g < G; ++g) {
        emax = egress[g] > emax ? egress[g] : emax;
        imax = ingress[g] > imax ? ingress[g] : imax;
    }
    return (double)(emax + imax) / G <= XG_RELAY_GAIN * (double)direct;
}

/* piece k of a relayed message of len bytes: [relay_cut(k), relay_cut(k + 1)), 16-B aligned cuts */
static int64_t relay_cut(int64_t len, int k, int G) { return k >= G ? len : ((len * k / G) & ~(int64_t)15); }

/* relay i (0 .. G-3) of a message from GPU gs to GPU gd: the GPUs other than gs, gd, ascending */
static int relay_gpu(int i, int gs, int gd)
{
    const int lo = gs < gd ? gs : gd, hi = gs < gd ? gd : gs;
    int h = i;
    if (h >= lo) ++h;
    if (h >= hi) ++h;
    return h;
}

static void relay_push(gvec *pp, int peer, int is_send, int buf, int64_t off, int64_t len, int group)
{
    xg_p2p *o;
    if (len <= 0) return;            /* a 0-byte piece (len < 16 G): no call on either side */
    o = ppush(pp);
    o->peer = peer; o->is_send = is_send; o->buf = buf; o->off = off; o->len = len; o->group = group;
}

/* GPU g's calls of one relayed step: group 0 = pieces 0 straight to the destination and pieces
 * 2 + i to relay R[i] (into its STAGE_RECV at *rbase on); group 1 = pieces 1 straight, and what g
 * holds as a relay forwarded to the destination.  Every list is in message order, so the k-th
 * send of any GPU to any other pairs with the k-th receive there, group by group -- and the relay
 * area is laid out in that order across GPU pairs: this walk is over the step, not over buckets. */
static void relay_calls(bcx *x, int b, int e)
{
    const int G = x->G, g = x->g;
    gvec *const pp = &x->pp;
    int grp, k, i;
    int64_t roff = x->rbase;
    for (grp = 0; grp < 2; ++grp) {
        roff = x->rbase;
        for (k = b; k < e; ++k) {
            const xg_msg *m = step_msg(x, k);
            const int c = msg_bucket(x, m), gs = c / G, gd = c % G;
            const int ri = g != gs && g != gd ? g - (g > gs) - (g > gd) : -1;   /* g's relay index */
            int64_t so, dof;
            if (c < 0 || gs == gd) continue;
            so = src_off(&x->pb, m);
            dof = dst_off(&x->pb, m);
            if (g == gs) {
                relay_push(pp, gd, 1, m->sbuf, so + relay_cut(m->len, grp, G),
                           relay_cut(m->len, grp + 1, G) - relay_cut(m->len, grp, G), grp);
                for (i = 0; grp == 0 && i < G - 2; ++i)
                    relay_push(pp, relay_gpu(i, gs, gd), 1, m->sbuf, so + relay_cut(m->len, 2 + i, G),
                               relay_cut(m->len, 3 + i, G) - relay_cut(m->len, 2 + i, G), 0);
            }
            if (ri >= 0) {
                const int64_t len = relay_cut(m->len, 3 + ri, G) - relay_cut(m->len, 2 + ri, G);
                if (grp == 0) relay_push(pp, gs, 0, XG_BUF_STAGE_RECV, roff, len, 0);
                else relay_push(pp, gd, 1, XG_BUF_STAGE_RECV, roff, len, 1);
                roff += len > 0 ? len : 0;
            }
            if (g == gd) {
                relay_push(pp, gs, 0, m->dbuf, dof + relay_cut(m->len, grp, G),
                           relay_cut(m->len, grp + 1, G) - relay_cut(m->len, grp, G), grp);
                for (i = 0; grp == 1 && i < G - 2; ++i)
                    relay_push(pp, relay_gpu(i, gs, gd), 0, m->dbuf, dof + relay_cut(m->len, 2 + i, G),
                               relay_cut(m->len, 3 + i, G) - relay_cut(m->len, 2 + i, G), 1);
            }
        }
    }
    x->rbase = roff;
}

/* ---- coalesced relay form (XG_RELAY_COALESCED, xg_sched.h): relay_step's steps, relay_cut's
 * pieces, relay_gpu's hops -- so every link carries what it carries in the relay form -- but one
 * RCCL call per (hop, kind) instead of one per piece.  RCCL serialises the calls of a group to
 * one peer at 2.7-4 us each (profiles/r06/relay_cost.log), and the relay form posts G calls per
 * message and direction: a pairwise round of 4 messages per GPU pair, 112 calls per GPU where
 * the direct form posts 8.  Here GPU g posts:
 *   group 0, per peer p: [pieces of g's messages to p that go straight (piece 0)],
 *                        [pieces of g's messages p relays, by destination];
 *            and receives the same two from p;
 *   group 1, per peer p: [g's own second pieces to p], then per source a (ascending): [the block
 *            of a's group-0 call that g relays to p] -- contiguous in g's STAGE_RECV, so it is
 *            forwarded as it lies; and receives the same from p.
 * A call of one piece moves in place (send from the segment, receive into the slot); a longer one
 * is packed into STAGE_SEND in the step's pre launch and unpacked out of STAGE_RECV after the
 * exchange (HBM copies, two orders of magnitude above a link's rate) -- unless its pieces average
 * >= XG_COALESCE_SPLIT: then it goes one call per piece, in place (rc_split).  STAGE_RECV holds the
 * unpacked receives from 0 on (the layout the device displacement scan rebuilds) and the relayed
 * blocks behind them.  A pairwise round: G - 1 sends + G - 1 receives per group. */
#define XG_WEIGHT_ONE 1024      /* a weighted step's shares: 1/1024ths of each GPU pair's bytes */

/* the piece of a message gs -> gd that travels via GPU h (relay_calls' assignment) */
static int rc_piece(int gs, int gd, int h) { return h == gd ? 0 : h == gs ? 1 : 2 + h - (h > gs) - (h > gd); }

/* cut at c / XG_WEIGHT_ONE of a message of len bytes, 16-B aligned (the last cut: len) */
static int64_t wcut(int64_t len, int c) { return c >= XG_WEIGHT_ONE ? len : ((len * c / XG_WEIGHT_ONE) & ~(int64_t)15); }

/* [lo, hi) of message m (a -> b) that travels via h: relay_cut's piece, or a weighted step's share,
 * the shares laid out in hop order (h = 0 .. G-1) */
static void rc_range(const bcx *x, const xg_msg *m, int a, int b, int h, int64_t *lo, int64_t *hi)
{
    if (x->w) {
        const int *w = &x->w[((size_t)a * x->G + b) * x->G];
        int c = 0, k;
        for (k = 0; k < h; ++k) c += w[k];
        *lo = wcut(m->len, c);
        *hi = w[h] ? wcut(m->len, c + w[h]) : *lo;
    } else {
        const int pi = rc_piece(a, b, h);
        *lo = relay_cut(m->len, pi, x->G);
        *hi = relay_cut(m->len, pi + 1, x->G);
    }
}

/* the pieces of the messages a -> b that travel via h (b < 0: every b other than a and h,
 * ascending), each message's in message order -> how many */
static int rc_collect(bcx *x, int a, int b, int h)
{
    const int G = x->G, b0 = b < 0 ? 0 : b, b1 = b < 0 ? G : b + 1;
    int n = 0, bb, k;
    for (bb = b0; bb < b1; ++bb) {
        if (bb == a || (b < 0 && bb == h)) continue;
        for (k = x->bk_off[a * G + bb]; k < x->bk_off[a * G + bb + 1]; ++k) {
            const xg_msg *m = &x->s->msgs[x->bk[k]];
            int64_t lo, hi;
            rc_range(x, m, a, bb, h, &lo, &hi);
            if (hi <= lo) continue;
            x->pm[n] = m; x->po[n] = lo; x->pl[n] = hi - lo; ++n;
        }
    }
    return n;
}

static int64_t rc_total(const bcx *x, int n)
{
    int64_t t = 0;
    int i;
    for (i = 0; i < n; ++i) t += x->pl[i];
    return t;
}

/* a call of n pieces goes one call per piece, in place, when its pieces are large: at >= 4 MiB a
 * piece an RCCL call (~3 us) costs less than packing and unpacking it (2 x its bytes of HBM traffic
 * at ~5 TB/s each way: >= 3 us) -- configs[4]'s 64 MiB segments, whose pieces are 8 MiB.  Both ends
 * of a call apply it to the same piece list, so the calls still pair one to one. */
#define XG_COALESCE_SPLIT ((int64_t)4 << 20)
static int rc_split(const bcx *x, int n) { return n > 1 && rc_total(x, n) >= XG_COALESCE_SPLIT * n; }

/* send the n collected pieces to peer in group grp: in place, or packed into STAGE_SEND */
static void rc_send(bcx *x, int n, int peer, int grp)
{
    int64_t t = 0;
    int i;
    if (!n || x->dry) return;
    if (n == 1 || rc_split(x, n)) {
        for (i = 0; i < n; ++i)
            relay_push(&x->pp, peer, 1, x->pm[i]->sbuf, src_off(&x->pb, x->pm[i]) + x->po[i], x->pl[i], grp);
        return;
    }
    for (i = 0; i < n; ++i) {
        xg_copy *c = cpush(&x->pre);
        c->src_buf = x->pm[i]->sbuf; c->src_off = src_off(&x->pb, x->pm[i]) + x->po[i];
        c->dst_buf = XG_BUF_STAGE_SEND; c->dst_off = x->sbase + t;
        c->len = x->pl[i];
        t += x->pl[i];
    }
    relay_push(&x->pp, peer, 1, XG_BUF_STAGE_SEND, x->sbase, t, grp);
    x->sbase += t;
}

/* receive the n collected pieces (all ending at this GPU) from peer: in place, or into the unpack
 * area of STAGE_RECV with one unpack copy per piece */
static void rc_recv(bcx *x, int n, int peer, int grp)
{
    int64_t t = 0;
    int i;
    if (!n) return;
    if (n == 1 || rc_split(x, n)) {
        for (i = 0; i < n && !x->dry; ++i)
            relay_push(&x->pp, peer, 0, x->pm[i]->dbuf, dst_off(&x->pb, x->pm[i]) + x->po[i], x->pl[i], grp);
        return;
    }
    for (i = 0; i < n && !x->dry; ++i) {
        xg_copy *c = cpush(&x->post);
        c->src_buf = XG_BUF_STAGE_RECV; c->src_off = x->ubase + t;
        c->dst_buf = x->pm[i]->dbuf; c->dst_off = dst_off(&x->pb, x->pm[i]) + x->po[i];
        c->len = x->pl[i];
        t += x->pl[i];
    }
    if (x->dry) t = rc_total(x, n);
    else relay_push(&x->pp, peer, 0, XG_BUF_STAGE_RECV, x->ubase, t, grp);
    x->ubase += t;
}

/* GPU g's calls of one relayed step (dry: only the unpack area's size, x->ubase) */
static void rc_step(bcx *x)
{
    const int G = x->G, g = x->g;
    int p, a, b, n;
    for (p = 0; p < G; ++p) {           /* group 0 */
        if (p == g) continue;
        rc_send(x, rc_collect(x, g, p, p), p, 0);
        rc_send(x, rc_collect(x, g, -1, p), p, 0);
        rc_recv(x, rc_collect(x, p, g, g), p, 0);
        n = rc_collect(x, p, -1, g);    /* what g relays for p: one receive into the relay area */
        if (n && !x->dry) {
            const int64_t at = x->rlbase + x->rl;
            int64_t t = 0;
            if (rc_split(x, n))         /* (or one per piece, as the sender splits them) */
                for (b = 0; b < n; ++b) {
                    relay_push(&x->pp, p, 0, XG_BUF_STAGE_RECV, at + t, x->pl[b], 0);
                    t += x->pl[b];
                }
            else
                relay_push(&x->pp, p, 0, XG_BUF_STAGE_RECV, at, rc_total(x, n), 0);
            for (t = 0, b = 0; b < G; ++b) {
                if (b == p || b == g) continue;
                x->blk[p * G + b] = at + t;
                t += rc_total(x, rc_collect(x, p, b, g));
            }
            x->rl += t;
        }
    }
    for (p = 0; p < G; ++p) {           /* group 1 */
        if (p == g) continue;
        rc_send(x, rc_collect(x, g, p, g), p, 1);
        for (a = 0; a < G && !x->dry; ++a)
            if (a != g && a != p && (n = rc_collect(x, a, p, g))) {
                /* the block of a's pieces for p, as it lies (one call, or one per piece) */
                int64_t at = x->blk[a * G + p];
                if (rc_split(x, n))
                    for (b = 0; b < n; at += x->pl[b], ++b) relay_push(&x->pp, p, 1, XG_BUF_STAGE_RECV, at, x->pl[b], 1);
                else
                    relay_push(&x->pp, p, 1, XG_BUF_STAGE_RECV, at, rc_total(x, n), 1);
            }
        rc_recv(x, rc_collect(x, p, g, p), p, 1);
        for (a = 0; a < G; ++a)
            if (a != g && a != p) rc_recv(x, rc_collect(x, a, g, p), p, 1);
    }
}

/* ---- weighted two-hop split (XG_RELAY_COALESCED on a step relay_step leaves direct).  A traffic
 * matrix that is not a permutation -- configs[4]'s m7 (mpi_test.c:942-997): every GPU sends 512 MiB
 * to each of 3-4 others per step, some GPUs receive from 4 -- gains nothing from the uniform cut
 * ((max egress + max ingress) / G is not below its busiest pair), yet a non-uniform one exists: the
 * best two-hop routing in two groups carries 0.78 of the direct form's busiest-link bytes
 * (profiles/r05/relay_lp.txt, an LP).  Per step, Frank-Wolfe on a soft-max of the busiest group-0
 * and group-1 links (profiles/relay_lp.py's fw_two_hop, here in C, 1000 iterations): every pair's bytes split over
 * its G paths -- straight in group 0 (h = b), straight in group 1 (h = a), via relay h -- starting
 * half straight in each group; each iteration moves 2 / (t + 3) of every pair onto its cheapest
 * path under the current gradient.  The best split seen is rounded to 1/1024ths (shares under
 * 16/1024 go to the pair's largest: each more hop is one more call), and the step is weighted
 * when its quantised link time is at
 * most XG_WEIGHTED_GAIN of the busiest pair's and every cross message is >= XG_RELAY_MIN_BYTES.
 * Deterministic: every GPU computes it from the same message list with the same code. */
#define XG_FW_ITERS 1000
#define XG_FW_SHARP 80.0
#define XG_WEIGHTED_GAIN 0.85

/* group-0 / group-1 link loads of split y (pairs pr[np][2], y[np][G] bytes) -> max l0 + max l1 */
static double fw_cost(int G, int np, const int *pr, const double *y, double *l0, double *l1)
{
    int i, h, k;
    double m0 = 0, m1 = 0;
    memset(l0, 0, sizeof(double) * (size_t)G * G);
    memset(l1, 0, sizeof(double) * (size_t)G * G);
    for (i = 0; i < np; ++i) {
        const int a = pr[2 * i], b = pr[2 * i + 1];
        for (h = 0; h < G; ++h) {
            if (h != a) l0[a * G + h] += y[i * G + h];
            if (h != b) l1[h * G + b] += y[i * G + h];
        }
    }
    for (k = 0; k < G * G; ++k) {
        m0 = l0[k] > m0 ? l0[k] : m0;
        m1 = l1[k] > m1 ? l1[k] : m1;
    }
    return m0 + m1;
}

/* The split is a pure function of the step's GPU-pair matrix, and every GPU's plan (each rank
 * builds all G of them for the pairing proof) asks for the same steps: a per-thread memo of the last
 * XG_FW_MEMO matrices (G <= 8), matched on the exact matrix, answers the repeats. */
#define XG_FW_MEMO 256
typedef struct { int G, rc; uint64_t key; double D[64]; int w[512]; } fw_memo;
static __thread fw_memo *fw_memo_tab;
static __thread unsigned fw_memo_next;

static uint64_t fw_key(const double *D, int n)
{
    uint64_t hsh = 1469598103934665603ull;
    int i;
    for (i = 0; i < n; ++i) {
        uint64_t v;
        memcpy(&v, &D[i], sizeof v);
        hsh = (hsh ^ v) * 1099511628211ull;
    }
    return hsh;
}

/* the memo entry of matrix D (G x G), or NULL */
static const fw_memo *fw_memo_find(const double *D, int G, uint64_t key)
{
    unsigned i;
    if (!fw_memo_tab || G > 8) return NULL;
    for (i = 0; i < XG_FW_MEMO; ++i)
        if (fw_memo_tab[i].G == G && fw_memo_tab[i].key == key &&
            !memcmp(fw_memo_tab[i].D, D, sizeof(double) * (size_t)G * G))
            return &fw_memo_tab[i];
    return NULL;
}

static void fw_memo_put(const double *D, int G, uint64_t key, const int *w, int rc)
{
    fw_memo *m;
    if (G > 8) return;
    if (!fw_memo_tab && !(fw_memo_tab = (fw_memo *)calloc(XG_FW_MEMO, sizeof(fw_memo)))) return;
    m = &fw_memo_tab[fw_memo_next++ % XG_FW_MEMO];
    m->G = G; m->rc = rc; m->key = key;
    memcpy(m->D, D, sizeof(double) * (size_t)G * G);
    memcpy(m->w, w, sizeof(int) * (size_t)G * G * G);
}

/* The weighted split of a step of pair[a * G + b] bytes (relay_step's, where it returns 0) into
 * w[(a * G + b) * G + h] (1/XG_WEIGHT_ONE) -> 1: weight the step, 0: it stays direct, -1: out of host memory */
static int weighted_step(const int64_t *pair, int G, int *w)
{
    uint64_t key = 0;
    const fw_memo *hit;
    int k, i, h, np = 0, t, rc = -1;
    double direct = 0, best = -1, cost;
    double *D = (double *)calloc((size_t)G * G, sizeof(double));
    int *pr = (int *)malloc(sizeof(int) * 2 * (size_t)G * G);
    double *y = (double *)calloc((size_t)G * G * G, sizeof(double)), *yb = (double *)calloc((size_t)G * G * G, sizeof(double));
    double *l0 = (double *)malloc(sizeof(double) * (size_t)G * G), *l1 = (double *)malloc(sizeof(double) * (size_t)G * G);
    double *g0 = (double *)malloc(sizeof(double) * (size_t)G * G), *g1 = (double *)malloc(sizeof(double) * (size_t)G * G);
    if (!D || !pr || !y || !yb || !l0 || !l1 || !g0 || !g1) goto done;
    rc = 0;
    for (i = 0; i < G * G; ++i) D[i] = (double)pair[i];     /* exact: sums of lengths, far below 2^53 */
    for (i = 0; i < G * G; ++i) {
        direct = D[i] > direct ? D[i] : direct;
        if (D[i] > 0) {
            pr[2 * np] = i / G;
            pr[2 * np + 1] = i % G;
            y[(size_t)np * G + i / G] = y[(size_t)np * G + i % G] = D[i] / 2;   /* half straight in each group */
            ++np;
        }
    }
    if (!np) goto done;
    key = fw_key(D, G * G);
    if ((hit = fw_memo_find(D, G, key))) {
        memcpy(w, hit->w, sizeof(int) * (size_t)G * G * G);
        rc = hit->rc;
        goto done;
    }
    for (t = 0; t <= XG_FW_ITERS; ++t) {
        double m0 = 0, m1 = 0, z0 = 0, z1 = 0, beta;
        cost = fw_cost(G, np, pr, y, l0, l1);
        if (best < 0 || cost < best) {
            best = cost;
            memcpy(yb, y, sizeof(double) * (size_t)np * G);
        }
        if (t == XG_FW_ITERS) break;
        for (k = 0; k < G * G; ++k) {
            m0 = l0[k] > m0 ? l0[k] : m0;
            m1 = l1[k] > m1 ? l1[k] : m1;
        }
        beta = XG_FW_SHARP / cost;
        for (k = 0; k < G * G; ++k) {       /* links far below the busiest weigh nothing (< e^-30) */
            const double e0 = beta * (l0[k] - m0), e1 = beta * (l1[k] - m1);
            g0[k] = e0 > -30.0 ? exp(e0) : 0.0;
            g1[k] = e1 > -30.0 ? exp(e1) : 0.0;
            z0 += g0[k];
            z1 += g1[k];
        }
        for (k = 0, z0 = 1.0 / z0, z1 = 1.0 / z1; k < G * G; ++k) {     /* soft-max weights */
            g0[k] *= z0;
            g1[k] *= z1;
        }
        for (i = 0; i < np; ++i) {
            const int a = pr[2 * i], bb = pr[2 * i + 1];
            const double step = 2.0 / (t + 3), dem = D[a * G + bb];
            int arg = 0;
            double cmin = 0;
            for (h = 0; h < G; ++h) {
                const double c = (h != a ? g0[a * G + h] : 0.0) + (h != bb ? g1[h * G + bb] : 0.0);
                if (h == 0 || c < cmin) { cmin = c; arg = h; }
            }
            for (h = 0; h < G; ++h) y[(size_t)i * G + h] += step * ((h == arg ? dem : 0.0) - y[(size_t)i * G + h]);
        }
    }
    /* quantise the best split: 1/1024ths, small shares folded into the pair's largest */
    memset(w, 0, sizeof(int) * (size_t)G * G * G);
    for (i = 0; i < np; ++i) {
        const int a = pr[2 * i], bb = pr[2 * i + 1];
        int *wp = &w[((size_t)a * G + bb) * G], sum = 0, big = 0;
        for (h = 0; h < G; ++h) {
            const int q = (int)(yb[(size_t)i * G + h] / D[a * G + bb] * XG_WEIGHT_ONE + 0.5);
            wp[h] = q >= 16 ? q : 0;
            sum += wp[h];
            if (wp[h] > wp[big]) big = h;
        }
        wp[big] += XG_WEIGHT_ONE - sum;
        for (h = 0; h < G; ++h) yb[(size_t)i * G + h] = D[a * G + bb] * wp[h] / XG_WEIGHT_ONE;
    }
    rc = fw_cost(G, np, pr, yb, l0, l1) <= XG_WEIGHTED_GAIN * direct;
    fw_memo_put(D, G, key, w, rc);
done:
    free(D); free(pr); free(y); free(yb); free(l0); free(l1); free(g0); free(g1);
    return rc;
}

/* the coalesced relay calls of the step (w: a weighted step's shares, or NULL): packs into pre, calls
 * into pp, unpacks into post, and the step's STAGE_SEND / STAGE_RECV bytes */
static void relay_coalesced_calls(bcx *x, const int *w)
{
    x->w = w; x->ubase = x->rl = 0; x->dry = 1;
    rc_step(x);                         /* the unpack area's size: the relay area goes behind it */
    x->rlbase = x->ubase; x->ubase = 0; x->dry = 0;
    rc_step(x);
    x->rbase = x->rlbase + x->rl;
}

/* ---- the parts of one step, in the order xg_devplan_build_form runs them.  What deals with a peer
 * takes a direction: OUT is the source end of bucket (g, p), STAGE_SEND and the pre copies, IN the
 * destination end of bucket (p, g), STAGE_RECV and the post copies -- a GPU's sends and its peer's
 * receives come from one body. */

/* rank-local memcpy's through SCRATCH first, in a launch of their own: the local copies and packs
 * of the step may read what they write in it */
static void step_stage_copies(bcx *x, int b, int e)
{
    int k;
    for (k = b; k < e; ++k) {
        const xg_msg *m = step_msg(x, k);
        if (moves(m) && is_stage(m) && xg_gpu_of(x->s->P, x->G, m->src) == x->g) local_copy(x, m);
    }
}

/* this GPU's local copies, and per direction and peer the bytes the pack decision goes by */
static void step_local_copies(bcx *x)
{
    int i, k, hi;
    for (k = peer_bucket(x, x->g, OUT, &hi); k < hi; ++k) local_copy(x, bk_msg(x, k));
    for (i = 0; i < 2 * x->G; ++i) {        /* i = dir * G + p */
        x->vol_b[i] = 0;
        for (k = peer_bucket(x, i % x->G, i / x->G, &hi); k < hi && i % x->G != x->g; ++k)
            x->vol_b[i] += bk_msg(x, k)->len;
    }
}

/* the relay decision, the same on every GPU: 0 = the step's messages go as they are, 1 = relayed in
 * relay_cut's uniform pieces, 2 = relayed in the weighted shares rl_w */
static int step_relay(bcx *x, int b, int e)
{
    int r;
    if (x->form != XG_RELAY && x->form != XG_RELAY_COALESCED) return 0;
    r = relay_step(x, b, e);
    if (r || x->form != XG_RELAY_COALESCED) return r > 0;
    /* a step the uniform cut does not help may still take a weighted two-hop split */
    r = weighted_step(x->rl_p, x->G, x->rl_w);
    x->oom |= r < 0;
    return r > 0 ? 2 : 0;
}

/* is the list exchanged with peer p in direction dir packed?  (both ends see the same list) */
static int packed(const bcx *x, int p, int dir)
{
    int hi, lo = peer_bucket(x, p, dir, &hi);
    return x->vol_b[dir * x->G + p] && use_pack(hi - lo, x->vol_b[dir * x->G + p], x->pack_max_seg, x->pack_min);
}

/* this GPU's end of message m: the source (OUT) or the destination (IN) */
static void msg_end(const bcx *x, const xg_msg *m, int dir, int32_t *buf, int64_t *off)
{
    *buf = dir == OUT ? m->sbuf : m->dbuf;
    *off = dir == OUT ? src_off(&x->pb, m) : dst_off(&x->pb, m);
}

/* the copy of message m between this GPU's end of it and staging at `at`: a pack into STAGE_SEND in
 * the pre launch (OUT), an unpack out of STAGE_RECV in the post launch (IN) */
static void stage_copy(bcx *x, int dir, const xg_msg *m, int64_t at)
{
    xg_copy *c = cpush(dir == OUT ? &x->pre : &x->post);
    if (dir == OUT) {
        msg_end(x, m, OUT, &c->src_buf, &c->src_off);
        c->dst_buf = XG_BUF_STAGE_SEND; c->dst_off = at;
    } else {
        c->src_buf = XG_BUF_STAGE_RECV; c->src_off = at;
        msg_end(x, m, IN, &c->dst_buf, &c->dst_off);
    }
    c->len = m->len;
}

/* is run r of a one-sided layout staged at this end?  The sender stages the runs of a
 * destination-ordered layout, the receiver those of a source-ordered one; the rest move as they lie */
static int os_staged(const oneside *o, int r, int dir) { return o->staged[r] && o->by_src == (dir == IN); }

/* the staged copies of the packed list of peer p, back to back from `at` on: every message of the
 * bucket (two-sided), or of the runs staged at this end (one-sided) -> their bytes */
static int64_t staged_copies(bcx *x, int p, int dir, int64_t at)
{
    const oneside *o = &x->os[dir * x->G + p];
    int64_t off = 0;
    int r, k, hi;
    if (x->form != XG_PACK_ONE_SIDED)
        for (k = peer_bucket(x, p, dir, &hi); k < hi; ++k) {
            stage_copy(x, dir, bk_msg(x, k), at + off);
            off += bk_msg(x, k)->len;
        }
    else
        for (r = 0; r < o->nrun; ++r)
            for (k = o->run_b[r]; k < o->run_b[r + 1] && os_staged(o, r, dir); ++k) {
                stage_copy(x, dir, os_msg(x->s, o, k), at + off);
                off += os_msg(x->s, o, k)->len;
            }
    return off;
}

/* packs (into staging) join the pre-exchange copy launch, those of all peers ahead of any call; a
 * coalesced relay's come with its calls and unpacks */
static void step_packs(bcx *x, int relayed)
{
    int p, dir, lo, hi;
    if (relayed && x->form == XG_RELAY_COALESCED) relay_coalesced_calls(x, relayed == 2 ? x->rl_w : NULL);
    for (p = 0; p < x->G; ++p) {
        /* the one-sided layout of every packed list of this GPU's, both directions */
        for (dir = OUT; dir <= IN && x->form == XG_PACK_ONE_SIDED; ++dir) {
            oneside *o = &x->os[dir * x->G + p];
            lo = peer_bucket(x, p, dir, &hi);
            if (packed(x, p, dir)) os_build(x->s, &x->pb, &x->bk[lo], hi - lo, o);
            x->oom |= o->fail;
        }
        if (packed(x, p, OUT)) x->sbase += staged_copies(x, p, OUT, x->sbase);
    }
}

/* one call of len bytes: at message m's end on this GPU, or (m NULL) at the staging region's fill */
static void peer_call(bcx *x, int p, int dir, const xg_msg *m, int64_t len)
{
    int64_t *fill = dir == OUT ? &x->soff : &x->rbase;
    xg_p2p *q = ppush(&x->pp);
    q->peer = p; q->is_send = dir == OUT; q->len = len;
    if (m) { msg_end(x, m, dir, &q->buf, &q->off); return; }
    q->buf = dir == OUT ? XG_BUF_STAGE_SEND : XG_BUF_STAGE_RECV; q->off = *fill;
    *fill += len;
}

/* direct: one call per message, at its end on this GPU */
static void direct_calls(bcx *x, int p, int dir)
{
    int k, hi;
    for (k = peer_bucket(x, p, dir, &hi); k < hi; ++k) peer_call(x, p, dir, bk_msg(x, k), bk_msg(x, k)->len);
}

/* two-sided: one call of the whole list in staging; the receiver unpacks every message */
static void two_sided_calls(bcx *x, int p, int dir)
{
    if (dir == IN) staged_copies(x, p, IN, x->rbase);
    peer_call(x, p, dir, NULL, x->vol_b[dir * x->G + p]);
}

/* one-sided: one call per run, in staging where this end stages it (the receiver unpacks those),
 * else where the run lies */
static void one_sided_calls(bcx *x, int p, int dir)
{
    const oneside *o = &x->os[dir * x->G + p];
    int r, k;
    if (dir == IN) staged_copies(x, p, IN, x->rbase);
    for (r = 0; r < o->nrun; ++r) {
        int64_t len = 0;
        for (k = o->run_b[r]; k < o->run_b[r + 1]; ++k) len += os_msg(x->s, o, k)->len;
        peer_call(x, p, dir, os_staged(o, r, dir) ? NULL : os_msg(x->s, o, o->run_b[r]), len);
    }
}

/* the grouped exchange: per peer, sends then receives, message order */
static void step_calls(bcx *x, int b, int e, int relayed)
{
    int p, dir;
    /* every message over all G - 1 links of its source, then of its destination (two groups) */
    if (relayed && x->form == XG_RELAY) relay_calls(x, b, e);
    for (p = 0; p < x->G; ++p)
        for (dir = OUT; dir <= IN; ++dir) {
            if (!x->vol_b[dir * x->G + p]) continue;
            *(dir == OUT ? &x->dp->remote_send_bytes : &x->dp->remote_recv_bytes) += x->vol_b[dir * x->G + p];
            if (relayed) continue;
            if (!packed(x, p, dir)) direct_calls(x, p, dir);
            else if (x->form == XG_PACK_ONE_SIDED) one_sided_calls(x, p, dir);
            else two_sided_calls(x, p, dir);
        }
    if (!relayed && x->soff != x->sbase && !x->oom) { fprintf(stderr, "xg_devplan_build: staging mismatch\n"); abort(); }
}

xg_devplan *xg_devplan_build_form(const xg_sched *s, int ngpus, int g, int64_t pack_max_seg, int64_t pack_min,
                                  int form)
{
    const int nst = s->nsteps, G = ngpus;
    int i, st;
    xg_devplan *dp;
    bcx x;
    bcx_init(&x, s, G, g, pack_max_seg, pack_min, form);
    dp = x.dp;
    if (x.oom) goto done;
    dp->gpu = g; dp->ngpus = G; dp->nsteps = nst; dp->flags = xg_sched_ragged(s) ? XG_DP_RAGGED : 0;
    /* per step, the request posts of this GPU's ranks (graph replays share their launch time out by
     * them: xg_plan_run) */
    xgi_step_posts_of(s, G, g, x.posts, nst);
    for (st = 0; st < nst; ++st) dp->steps[st].posts = x.posts[st];
    /* in-loop MPI_Barrier -> device-side barrier after the step it completes at (G > 1) */
    for (i = 0; i < s->nbarrier; ++i)
        if (G > 1 && s->barrier_epoch[i] >= 0 && s->barrier_epoch[i] < nst) dp->steps[s->barrier_epoch[i]].sync_after = 1;
    dp->region_bytes[XG_BUF_SEND] = xg_region_bytes(s, G, g, XG_BUF_SEND);
    dp->region_bytes[XG_BUF_RECV] = xg_region_bytes(s, G, g, XG_BUF_RECV);
    dp->region_bytes[XG_BUF_SCRATCH] = xg_region_bytes(s, G, g, XG_BUF_SCRATCH);
    for (st = 0; st < nst && !x.oom; ++st) {
        const int b = x.cnt[st], e = x.cnt[st + 1];
        xg_stepplan *sp = &dp->steps[st];
        int relayed;
        x.sbase = x.rbase = x.soff = 0;
        sp->pre_begin = x.pre.n; sp->p2p_begin = x.pp.n; sp->post_begin = x.post.n;
        step_index(&x, b, e);
        step_stage_copies(&x, b, e);
        sp->stage_count = x.pre.n - sp->pre_begin;
        step_local_copies(&x);
        relayed = step_relay(&x, b, e);
        step_packs(&x, relayed);
        sp->pre_count = x.pre.n - sp->pre_begin;
        step_calls(&x, b, e, relayed);
        sp->p2p_count = x.pp.n - sp->p2p_begin;
        sp->post_count = x.post.n - sp->post_begin;
        if (x.sbase > dp->region_bytes[XG_BUF_STAGE_SEND]) dp->region_bytes[XG_BUF_STAGE_SEND] = x.sbase;
        if (x.rbase > dp->region_bytes[XG_BUF_STAGE_RECV]) dp->region_bytes[XG_BUF_STAGE_RECV] = x.rbase;
        for (i = 0; i < 2 * G; ++i) os_free(&x.os[i]);
    }
    /* post copies are stored after the pre copies in one array */
    x.oom |= x.pre.fail | x.post.fail | x.pp.fail;
    dp->ncopy = x.pre.n + x.post.n;
    if (!x.oom && (dp->copies = (xg_copy *)malloc(sizeof(xg_copy) * (dp->ncopy + 1)))) {
        if (x.pre.n) memcpy(dp->copies, x.pre.v, sizeof(xg_copy) * x.pre.n);
        if (x.post.n) memcpy(dp->copies + x.pre.n, x.post.v, sizeof(xg_copy) * x.post.n);
        for (st = 0; st < nst; ++st) dp->steps[st].post_begin += x.pre.n;
        dp->np2p = x.pp.n;
        dp->p2p = x.pp.v ? (xg_p2p *)x.pp.v : (xg_p2p *)malloc(sizeof(xg_p2p));
        if (dp->p2p == x.pp.v) x.pp.v = NULL;       /* owned by the plan now */
    }
    x.oom |= !dp->copies || !dp->p2p;
done:
    bcx_free(&x);
    if (x.oom) {
        xg_devplan_free(dp);
        return NULL;
    }
    return dp;
}

/* ------------------------------------------------------------------ fill / verify descriptors */
int xg_fill_runs(const xg_sched *s, int ngpus, int g, xg_segrun *out)
{
    int lo, hi, r, n = 0;
    xg_block_range(s->P, ngpus, g, &lo, &hi);
    for (r = lo; r < hi; ++r) {
        int ns = xgi_nsend_segs(s, r);
        if (!ns) continue;
        if (out) {   /* prepare_*_data: segment i of rank r carries seed i (:106-110, :195-199) */
            out[n].rank = r; out[n].seed0 = 0; out[n].nsegs = ns; out[n].pad = 0;
            out[n].off = xg_send_offset(s, ngpus, r);
        }
        n++;
    }
    return n;
}

int xg_verify_slots(const xg_sched *s, int ngpus, int g, xg_slot *out)
{
    int lo, hi, r, i, n = 0;
    xg_block_range(s->P, ngpus, g, &lo, &hi);
    for (r = lo; r < hi; ++r) {
        int nslots = xgi_nrecv_slots(s, r), myindex = 0;
        int64_t base;
        if (!nslots) continue;
        base = xg_recv_offset(s, ngpus, r);
        for (i = 0; i < s->A; ++i)
            if (s->rank_list[i] == r) myindex = i;
        for (i = 0; i < nslots; ++i, ++n) {
            if (!out) continue;
            /* check_buffer call sites: a2m (src=i, seed=myindex) :215; m2a (src=rank_list[i], seed=rank) :139 */
            out[n].src = s->dir == XG_A2M ? i : s->rank_list[i];
            out[n].seed = s->dir == XG_A2M ? myindex : r;
            out[n].dst = r; out[n].pad = 0;
            out[n].off = base + xg_slot_offset(s, r, i);
        }
    }
    return n;
}

int xg_deliveries(const xg_sched *s, int ngpus, xg_delivery *out)
{
    int g, lo, hi, r, i, n = 0;
    for (g = 0; g < ngpus; ++g) {
        xg_block_range(s->P, ngpus, g, &lo, &hi);
        for (r = lo; r < hi; ++r) {          /* xg_verify_slots' order and pairing */
            int nslots = xgi_nrecv_slots(s, r), myindex = 0;
            if (!nslots) continue;
            for (i = 0; i < s->A; ++i)
                if (s->rank_list[i] == r) myindex = i;
            for (i = 0; i < nslots; ++i, ++n) {
                xg_delivery *q = out ? &out[n] : NULL;
                if (!q) continue;
                q->src = s->dir == XG_A2M ? i : s->rank_list[i];
                q->seed = s->dir == XG_A2M ? myindex : r;
                q->dst = r; q->slot = i;
                q->src_gpu = xg_gpu_of(s->P, ngpus, q->src); q->dst_gpu = g;
                q->send_off = xg_send_offset(s, ngpus, q->src) + xg_seg_offset(s, q->src, q->seed);
                q->recv_off = xg_recv_offset(s, ngpus, r) + xg_slot_offset(s, r, i);
            }
        }
    }
    return n;
}

int xg_delivery_lens(const xg_sched *s, int ngpus, int64_t *out)
{
    int g, lo, hi, r, i, n = 0;
    for (g = 0; g < ngpus; ++g) {
        xg_block_range(s->P, ngpus, g, &lo, &hi);
        for (r = lo; r < hi; ++r) {          /* xg_deliveries' order */
            const int nslots = xgi_nrecv_slots(s, r);
            for (i = 0; i < nslots; ++i, ++n)
                if (out) out[n] = xg_slot_offset(s, r, i + 1) - xg_slot_offset(s, r, i);
        }
    }
    return n;
}
