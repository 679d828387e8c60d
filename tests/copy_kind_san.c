/* The kernel kind of a copy launch (xg_copy_launch_choose) and the local-copies-meet-unpacks test
 * (xg_step_local_meets_unpacks), both of csrc/host/pieces.c, over the table cases of
 * tests/test_copy_kind.py and tests/test_pieces.py and over seeded random launches, CPU only.
 * Built by tests/test_copy_kind.py with pieces.c as ONE standalone executable under
 * -fsanitize=address,undefined (nothing preloaded): a read past the lengths array or the interval
 * tables, an overflow or a leak aborts the run. */
#include "xg_sched.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define KB ((int64_t)1 << 10)
#define MB ((int64_t)1 << 20)
enum { S = XG_BUF_SEND, R = XG_BUF_RECV, SS = XG_BUF_STAGE_SEND, SR = XG_BUF_STAGE_RECV };

static int fails;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) {                                                     \
            printf("line %d: %s\n", __LINE__, #x);                      \
            ++fails;                                                    \
        }                                                               \
    } while (0)

static xg_copy_rules defaults(void)
{
    xg_copy_rules r;
    memset(&r, 0, sizeof r);
    r.chunk = 32768; r.wave_min = MB; r.wave_max = 32 * MB; r.wg_cost = 2048; r.extent_mean_max = 1024;
    r.small_piece_min = 112 * MB; r.cus = 256; r.ragged_copy = r.extent_copy = r.small_pieces = 1;
    r.small_kib = r.small_order = 8;
    return r;
}

/* n copies of len bytes (the last of `last`) S -> dst_buf, back to back on the 16-B grid + phase */
static xg_copy_choice choose(int n, int64_t len, int64_t last, int phase, int dst_buf, int flags, int cross,
                             int may_small, int nt_cut, int nt_run, const xg_copy_rules *r, int *rc)
{
    xg_launch_facts f;
    xg_copy_choice ch;
    int64_t *lens = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1)), off = 0;
    int i;
    if (!lens) exit(2);
    memset(&f, 0, sizeof f);
    memset(&ch, 0xff, sizeof ch);
    for (i = 0; i < n; ++i) {
        xg_copy c;
        c.len = lens[i] = i == n - 1 ? last : len;
        c.src_off = off + phase; c.dst_off = off; c.src_buf = S; c.dst_buf = dst_buf;
        xg_launch_facts_add(&f, &c);
        off += (c.len > 0 ? (c.len + 15) / 16 * 16 : 0) + 16;
    }
    f.lens = lens; f.nlens = n; f.dp_flags = flags; f.cross = cross; f.may_small = may_small;
    f.nt_cut = nt_cut; f.nt_run = nt_run;
    *rc = xg_copy_launch_choose(&f, r, &ch);
    free(lens);
    return ch;
}

static void kind_table(void)
{
    xg_copy_rules r = defaults(), q;
    xg_copy_choice ch;
    int rc;
    const int both = XG_DP_RAGGED | XG_DP_EXTENTS;
    ch = choose(16, 64 * KB, 64 * KB, 0, R, 0, 1, 0, 0, 0, &r, &rc);                  /* bytes = wave_min */
    CHECK(rc == 0 && ch.kind == XG_COPY_WAVE && ch.kib == 2 && ch.piece == 2 * KB && !ch.nt);
    q = r; q.wave_min = MB + 1;
    CHECK(choose(16, 64 * KB, 64 * KB, 0, R, 0, 1, 0, 0, 0, &q, &rc).kind == XG_COPY_PIECE);
    q = r; q.wave_max = MB - 1;
    CHECK(choose(16, 64 * KB, 64 * KB, 0, R, 0, 1, 0, 0, 0, &q, &rc).kind == XG_COPY_PIECE);
    CHECK(choose(1, 8 * MB, 8 * MB, 0, R, 0, 1, 0, 0, 0, &r, &rc).kib == 8);
    CHECK(choose(1, 4 * MB, 4 * MB, 0, R, 0, 1, 0, 0, 0, &r, &rc).kib == 4);
    CHECK(choose(1, 4 * MB, 4 * MB - 16, 0, R, 0, 1, 0, 0, 0, &r, &rc).kib == 2);
    ch = choose(16, 256 * KB, 256 * KB, 0, R, 0, 1, 1, 0, 1, &r, &rc);                /* cut plain, run non-temporal */
    CHECK(ch.kind == XG_COPY_PIECE && ch.nt == 1 && ch.kib == 0 && ch.piece == 4 * KB);
    q = r; q.small_piece_min = 0;
    ch = choose(16, 256 * KB, 256 * KB, 0, R, 0, 1, 1, 0, 1, &q, &rc);
    CHECK(ch.kind == XG_COPY_SMALL && ch.nt == 1 && ch.kib == 8 && ch.order == 8 && ch.piece == 8 * KB);
    CHECK(choose(16, 256 * KB, 256 * KB, 0, R, 0, 1, 1, 0, 0, &q, &rc).kind == XG_COPY_WAVE);
    CHECK(choose(10, 1024, 1024, 3, R, both, 0, 0, 0, 0, &r, &rc).kind == XG_COPY_EXTENT);
    CHECK(choose(10, 1024, 1025, 3, R, both, 0, 0, 0, 0, &r, &rc).kind == XG_COPY_SHIFT);
    q = r; q.extent_copy = 0;
    CHECK(choose(10, 1024, 1024, 3, R, both, 0, 0, 0, 0, &q, &rc).kind == XG_COPY_SHIFT);
    CHECK(choose(10, 1024, 1024, 3, R, 0, 0, 0, 0, 0, &r, &rc).kind == XG_COPY_PIECE);
    q = r; q.ragged_copy = 0;
    CHECK(choose(10, 1024, 1024, 3, R, XG_DP_RAGGED, 0, 0, 0, 0, &q, &rc).kind == XG_COPY_PIECE);
    CHECK(choose(112, MB, MB, 0, R, 0, 0, 1, 1, 1, &r, &rc).kind == XG_COPY_SMALL);   /* = small_piece_min */
    CHECK(choose(112, MB, MB - 16, 0, R, 0, 0, 1, 1, 1, &r, &rc).kind == XG_COPY_PIECE);
    q = r; q.small_piece_min = 0;
    CHECK(choose(7, MB, MB + 16, 0, R, 0, 0, 1, 0, 0, &q, &rc).kind == XG_COPY_PIECE);    /* not uniform */
    CHECK(choose(7, MB, MB, 0, SS, 0, 0, 1, 0, 0, &q, &rc).kind == XG_COPY_PIECE);        /* packs */
    q.small_order = 1;
    CHECK(choose(511, 8 * KB << 22, 8 * KB << 22, 0, R, 0, 0, 1, 1, 1, &q, &rc).kind == XG_COPY_SMALL);
    CHECK(choose(512, 8 * KB << 22, 8 * KB << 22, 0, R, 0, 0, 1, 1, 1, &q, &rc).kind == XG_COPY_PIECE);
    q.small_order = 512;
    CHECK(choose(1, 8 * KB << 22, 8 * KB << 22, 0, R, 0, 0, 1, 1, 1, &q, &rc).kind == XG_COPY_PIECE);
    choose(3, 0, 0, 0, R, 0, 1, 1, 0, 0, &r, &rc);                                    /* no bytes: refused */
    CHECK(rc == -1);
    CHECK(xg_copy_launch_choose(NULL, &r, &ch) == -1);
}

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 11) % n);
}

static void kind_random(int rounds)
{
    static const int64_t lens[] = {16, 1000, 1024, 4096, 4097, 8 * 1024 + 16, 65536, 1 << 20};
    int i, rc, seen[XG_COPY_NKIND] = {0};
    for (i = 0; i < rounds; ++i) {
        xg_copy_rules r = defaults();
        xg_copy_choice ch;
        const int64_t len = lens[rnd(8)];
        r.wave_min = rnd(2) ? 0 : MB; r.small_piece_min = rnd(2) ? 0 : MB; r.cus = rnd(2) ? 64 : 256;
        r.wave_kib = rnd(4) ? 0 : 4; r.small_kib = rnd(2) ? 4 : 8; r.small_order = 1 + (int)rnd(32);
        ch = choose(1 + (int)rnd(50), len, rnd(3) ? len : lens[rnd(8)], rnd(4) ? 0 : (int)rnd(16), rnd(8) ? R : SS,
                    (int)rnd(4), (int)rnd(2), (int)rnd(2), (int)rnd(2), (int)rnd(2), &r, &rc);
        CHECK(rc == 0 && ch.kind >= 0 && ch.kind < XG_COPY_NKIND && ch.piece >= 2 * KB);
        CHECK((ch.kib != 0) == (ch.kind == XG_COPY_WAVE || ch.kind == XG_COPY_SMALL));
        CHECK(ch.kind != XG_COPY_WAVE || !ch.nt);
        seen[ch.kind]++;
    }
    for (i = 0; i < XG_COPY_NKIND; ++i) CHECK(seen[i] > 0);
}

/* step 0: unpacks `unp`; step 1: one local copy, then one pack */
static int meets(const xg_copy *unp, int nunp, xg_copy local)
{
    xg_copy copies[8];
    xg_stepplan st[2];
    xg_devplan dp;
    memset(st, 0, sizeof st);
    memset(&dp, 0, sizeof dp);
    copies[0] = local;
    copies[1].src_buf = S; copies[1].src_off = 0; copies[1].dst_buf = SS; copies[1].dst_off = 0; copies[1].len = 8;
    memcpy(copies + 2, unp, sizeof(xg_copy) * (size_t)nunp);
    st[0].post_begin = 2; st[0].post_count = nunp;
    st[1].pre_begin = 0; st[1].pre_count = 2;
    dp.ngpus = 2; dp.nsteps = 2; dp.ncopy = 2 + nunp; dp.copies = copies; dp.steps = st;
    return xg_step_local_meets_unpacks(&dp, 1);
}

static xg_copy cp(int sb, int64_t so, int db, int64_t d_o, int64_t n)
{
    xg_copy c;
    c.src_buf = sb; c.src_off = so; c.dst_buf = db; c.dst_off = d_o; c.len = n;
    return c;
}

static void meets_table(void)
{
    xg_copy unp[3], none[2];
    xg_devplan dp;
    unp[0] = cp(SR, 0, R, 1000, 100); unp[1] = cp(SR, 100, R, 1010, 20); unp[2] = cp(SR, 200, R, 5000, 50);
    none[0] = cp(SR, 0, R, 1000, 0); none[1] = cp(SR, 0, R, 5000, 0);
    CHECK(meets(unp, 3, cp(S, 0, R, 2000, 64)) == 0);
    CHECK(meets(unp, 3, cp(S, 0, R, 1099, 1)) == 1);      /* an unpack's last byte */
    CHECK(meets(unp, 3, cp(R, 1099, S, 0, 1)) == 1);
    CHECK(meets(unp, 3, cp(S, 0, R, 1100, 1)) == 0);      /* the byte after it */
    CHECK(meets(unp, 3, cp(R, 1100, S, 0, 8)) == 0);
    CHECK(meets(unp, 3, cp(S, 0, R, 900, 100)) == 0);
    CHECK(meets(unp, 3, cp(S, 0, R, 4000, 1001)) == 1);
    CHECK(meets(unp, 3, cp(R, 5049, S, 0, 8)) == 1);
    CHECK(meets(unp, 3, cp(S, 0, 7, 1000, 8)) == 0);      /* a region that does not exist meets nothing */
    CHECK(meets(unp, 0, cp(S, 0, R, 1000, 100)) == 0);    /* no unpacks */
    CHECK(meets(none, 2, cp(S, 0, R, 1000, 100)) == 0);   /* only empty ones */
    memset(&dp, 0, sizeof dp);
    dp.nsteps = 1;
    CHECK(xg_step_local_meets_unpacks(&dp, 0) == -1 && xg_step_local_meets_unpacks(&dp, 1) == -1);
    CHECK(xg_step_local_meets_unpacks(NULL, 1) == -1);
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
    kind_table();
    kind_random(rounds);
    meets_table();
    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("ok after %d launches\n", rounds);
    return 0;
}
