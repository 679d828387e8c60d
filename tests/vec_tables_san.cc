// vec_tables_san.cc -- a stand-alone program for the sanitizers (test_vec_tables.py compiles it with
// csrc/host/vec_tables.cc and the C host sources under -fsanitize=address,undefined and runs it):
// builds the row-launch tables of hand-made rows and of a vec list's rows (xg_vec_rows_build) at
// several tile sizes and launch caps, walks every dispatch, tile and lane with xg_vec_piece_at and
// checks, over the tables themselves, that the pieces are exactly the rows' blocks cut at the tile
// size, that the cuts obey their rule, that bad rows are refused and that a row of 2^30 blocks costs
// nothing.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vec_tables.h"

#define CHECK(x)                                                                    \
    do {                                                                            \
        if (!(x)) {                                                                 \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #x, g_what); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

static char g_what[256];
static int g_launches = 0;

static void regions_of(const std::vector<xg_vrow> &rows, uint64_t *base, int64_t *bytes)
{
    for (int b = 0; b < XG_NBUF; ++b) {
        base[b] = (uint64_t)(b + 1) << 44;
        bytes[b] = 0;
    }
    for (const xg_vrow &r : rows) {
        bytes[r.src_buf] = std::max(bytes[r.src_buf], r.src_off + (r.count - 1) * r.src_step + r.len);
        bytes[r.dst_buf] = std::max(bytes[r.dst_buf], r.dst_off + (r.count - 1) * r.dst_step + r.len);
    }
}

// walk == false: only the cut rule (a launch too large to walk)
static void check_launch(const std::vector<xg_vrow> &rows, int64_t tb, int tp, int64_t cap, bool walk)
{
    uint64_t base[XG_NBUF];
    int64_t bytes[XG_NBUF];
    regions_of(rows, base, bytes);
    xg_vec_tables *t = nullptr;
    CHECK(xg_vec_tables_build(rows.data(), (int64_t)rows.size(), base, bytes, tb, tp, cap, &t) == XG_OK && t);
    const int64_t T = xg_vec_tables_tiles(t), B = xg_vec_tables_bytes(t);
    const int nd = xg_vec_tables_dispatches(t);
    CHECK((int64_t)t->tile0.size() == (int64_t)rows.size() + 1 && t->tile0[0] == 0 && t->tile0.back() == T);
    CHECK(xg_vec_tables_cut(t, 0) == 0 && xg_vec_tables_cut(t, nd) == T && xg_vec_tables_cut(t, nd + 1) == -1);
    if (cap == 0 || B <= cap + cap / 2) CHECK(nd == (T > 0));
    int64_t sum = 0;
    for (int d = 0; d < nd; ++d) {
        const int64_t b = xg_vec_tables_cut(t, d), e = xg_vec_tables_cut(t, d + 1), nb = xg_vec_tables_dispatch_bytes(t, d);
        CHECK(b < e && nb > 0);
        if (d + 1 < nd) CHECK(nb >= cap);
        else if (nd > 1) CHECK(e - b >= 16 && nb >= cap / 2);
        sum += nb;
    }
    CHECK(sum == B);
    if (walk) {
        // every lane of every tile of every dispatch, against the rows' blocks in order
        size_t k = 0;           // the block the walk expects next: row k, block j, byte o of it
        int64_t j = 0, o = 0;
        for (int d = 0; d < nd; ++d) {
            int64_t nb = 0, last = 0;
            for (int64_t tile = xg_vec_tables_cut(t, d); tile < xg_vec_tables_cut(t, d + 1); ++tile) {
                size_t r = 0;
                while (t->tile0[r + 1] <= tile) ++r;
                const xgk::DVRow &w = t->rows[r];
                last = 0;
                for (int lane = 0; lane < tp; ++lane) {
                    const xg_vec_at p = xg_vec_piece_at(0, 0, w.src_step, w.dst_step, w.len, w.count, tb, tp,
                                                        tile - t->tile0[r], lane);
                    if (!p.n) continue;
                    CHECK(k < rows.size() && r == k);
                    const xg_vrow &x = rows[k];
                    const int64_t ss = x.count > 1 ? x.src_step : 0, ds = x.count > 1 ? x.dst_step : 0;
                    CHECK((uint64_t)(uintptr_t)w.src + (uint64_t)p.src_off == base[x.src_buf] + (uint64_t)(x.src_off + j * ss + o));
                    CHECK((uint64_t)(uintptr_t)w.dst + (uint64_t)p.dst_off == base[x.dst_buf] + (uint64_t)(x.dst_off + j * ds + o));
                    CHECK(p.n == std::min(tb, x.len - o));
                    nb += p.n; last += p.n;
                    o += p.n;
                    if (o == x.len) { o = 0; ++j; }
                    if (j == x.count) { j = 0; ++k; }
                }
            }
            CHECK(nb == xg_vec_tables_dispatch_bytes(t, d));
            if (d + 1 < nd) CHECK(nb < cap + last);         // at most one tile over the cap
        }
        CHECK(k == rows.size() && j == 0 && o == 0);
    }
    const int64_t n = xg_vec_tables_dump(t, nullptr, 0);
    std::vector<char> text((size_t)n + 1);
    CHECK(xg_vec_tables_dump(t, text.data(), n + 1) == n && text[n] == 0);
    xg_vec_tables_free(t);
    ++g_launches;
}

static void check_refused(xg_vrow r, int64_t region)
{
    uint64_t base[XG_NBUF] = {1ull << 44, 2ull << 44, 0, 0, 0};
    int64_t bytes[XG_NBUF] = {region, region, 0, 0, 0};
    xg_vec_tables *t = (xg_vec_tables *)1;
    CHECK(xg_vec_tables_build(&r, 1, base, bytes, 32768, 256, 0, &t) == XG_EARG && t == nullptr);
}

int main()
{
    static const int64_t tbs[] = {32768, 64};
    static const int tps[] = {256, 1};
    const int S = XG_BUF_SEND, R = XG_BUF_RECV;
    std::vector<xg_vrow> hand = {
        {S, R, 0, 3, 16, 37, 16, 700},          {S, R, 11200, 30000, 1000, 1003, 1000, 40},
        {S, R, 52000, 80000, 0, 0, 1, 1},       {S, R, 52001, 80001, 32768, 32771, 32768, 2},
        {S, R, 120000, 150000, 32784, 32784, 32784, 2}, {S, R, 190000, 220000, 100000, 100001, 100000, 3},
        {S, R, 500000, 530000, 65, 65, 65, 129},
        {S, R, 600000, 700000, 4099, ((int64_t)1 << 31) + 48, 4096, 3},      // block offsets past 2^31
        {S, R, 700000, 800000, ((int64_t)1 << 32) + 16, 4101, 4096, 2},
    };
    for (int64_t tb : tbs)
        for (int tp : tps)
            for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)700, (int64_t)4096, (int64_t)65536, (int64_t)1 << 40}) {
                snprintf(g_what, sizeof g_what, "hand tb %lld tp %d cap %lld", (long long)tb, tp, (long long)cap);
                check_launch(hand, tb, tp, cap, true);
            }
    // a striped view and its neighbours through the schedule: xg_vec_rows_build's rows on 1 and 2 GPUs
    {
        const int P = 6, A = 3;
        int rl[A];
        xg_aggregator_list(P, A, 1, 1, rl);
        std::vector<xg_vec> v;
        int64_t dom[A];
        for (int a = 0; a < A; ++a) {
            const int64_t L[3] = {64, 7, 300}, Sd = 64 + 7 + 300 + 5;
            int64_t at = 13 * a;
            for (int i = 0; i < 3; ++i) {
                v.push_back({(a + i) % P, a, at, L[i], Sd, 37 + a});
                at += L[i] + (i == 1 ? 5 : 0);
            }
            const int64_t hull = 13 * a + (36 + a) * Sd + Sd;
            v.push_back({(a + 4) % P, a, hull, 40000, 0, 1});
            v.push_back({(a + 5) % P, a, hull + 40000, 33, 33, 500});
            v.push_back({0, a, 0, 0, 5, 9});
            dom[a] = hull + 40000 + 33 * 500 + a;
        }
        char err[256] = "";
        CHECK(xg_vecs_check(v.data(), (int64_t)v.size(), P, A, dom, 1, err, sizeof err) == XG_OK);
        std::vector<int64_t> lens((size_t)P * A, 0);
        CHECK(xg_vecs_lens(v.data(), (int64_t)v.size(), P, A, lens.data()) == 0);
        for (int m : {1, 2}) {
            xg_sched *s = xg_sched_build_v(m, P, A, lens.data(), 2, rl, 1, 1, 0, 65424, 0, err, sizeof err);
            CHECK(s);
            for (int G : {1, 2})
                for (int g = 0; g < G; ++g) {
                    const int64_t n = xg_vec_rows_build(s, G, g, v.data(), (int64_t)v.size(), dom, nullptr, nullptr, nullptr);
                    CHECK(n >= 0);
                    std::vector<xg_vrow> rows((size_t)n);
                    CHECK(xg_vec_rows_build(s, G, g, v.data(), (int64_t)v.size(), dom, rows.data(), nullptr, nullptr) == n);
                    for (int64_t tb : tbs)
                        for (int tp : tps)
                            for (int64_t cap : {(int64_t)0, (int64_t)1000, (int64_t)30000}) {
                                snprintf(g_what, sizeof g_what, "vecs m %d G %d g %d tb %lld tp %d cap %lld", m, G, g,
                                         (long long)tb, tp, (long long)cap);
                                check_launch(rows, tb, tp, cap, true);
                            }
                }
            xg_sched_free(s);
        }
    }
    // the states of the cutting rule: a full dispatch behind which no cut is allowed; 2^30 blocks
    {
        const int64_t T16 = 256 * 64;
        snprintf(g_what, sizeof g_what, "cut states");
        check_launch({{S, R, 0, 0, 65, 67, 64, 256 * 148}}, 32768, 256, 64 * T16, true);
        check_launch({{S, R, 0, 0, 65, 67, 64, 256 * 64}, {S, R, 2000000, 2000000, 32768, 32768, 32768, 10}}, 32768, 256,
                     32 * T16, true);
        check_launch({{S, R, 0, 0, 65, 67, 64, 256 * 96}}, 32768, 256, 64 * T16, true);
        check_launch({{S, R, 0, 0, 65, 67, 64, 256 * 97}}, 32768, 256, 64 * T16, true);
        check_launch({{S, R, 0, 0, 16, 16, 16, (int64_t)1 << 30}}, 32768, 256, (int64_t)512 << 20, false);
        check_launch({{S, R, 0, 0, 16, 16, 16, (int64_t)1 << 30}}, 64, 1, (int64_t)512 << 20, false);
        check_launch({}, 32768, 256, 4096, true);
    }
    // refusals
    {
        const int64_t big = (int64_t)1 << 40;
        snprintf(g_what, sizeof g_what, "refusals");
        check_refused({S, R, 0, 0, 8, 8, 0, 4}, big);
        check_refused({S, R, 0, 0, 8, 8, 8, 0}, big);
        check_refused({S, R, 0, 0, 8, 8, 8, -1}, big);
        check_refused({S, R, 0, big - 100 - 2 * 50 + 1, 100, 50, 100, 3}, big);
        check_refused({S, R, big - 99, 0, 0, 0, 100, 1}, big);
        check_refused({S, R, 0, -1, 100, 100, 100, 3}, big);
        check_refused({S, R, 0, 150, 100, -100, 100, 3}, big);
        check_refused({S, R, 0, 0, 100, (int64_t)1 << 62, 100, 5}, big);
        check_refused({S, R, INT64_MAX - 50, 0, 0, 0, 100, 1}, big);
        check_refused({S, R, 0, 0, (int64_t)1 << 61, 16, 16, 9}, big);
        check_refused({S, R, 0, 0, 0, 0, big, (int64_t)1 << 30}, big);
        check_refused({S, 5, 0, 0, 8, 8, 8, 2}, big);
        check_refused({S, R, 0, 0, 1, 1, 1, ((int64_t)1 << 31) * 256 + 1}, big);       // more than INT32_MAX tiles
    }
    printf("%d launches covered\n", g_launches);
    return g_launches > 80 ? 0 : 1;
}
