// view_tables_san.cc -- a stand-alone program for the sanitizers (test_vec_views.py compiles it with
// csrc/host/vec_tables.cc and the C host sources under -fsanitize=address,undefined and runs it):
// recognises the views of hand-made and of a schedule's row lists in several list orders
// (xg_vrow_views), builds their view-launch tables (xg_view_tables_build) at several tile sizes and
// launch caps, walks every dispatch, tile and lane with xg_view_piece_at and xg_view_piece and checks,
// over the tables themselves, that the pieces are exactly the rows' blocks cut at the tile size, each
// once, that a tile's pieces ascend across the rows of its view, that the cuts obey their rule, that
// bad rows are refused and that a view of 2^30 blocks costs nothing.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <tuple>
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
        const int64_t ss = r.count > 1 ? r.src_step : 0, ds = r.count > 1 ? r.dst_step : 0;
        bytes[r.src_buf] = std::max(bytes[r.src_buf], r.src_off + (r.count - 1) * ss + r.len);
        bytes[r.dst_buf] = std::max(bytes[r.dst_buf], r.dst_off + (r.count - 1) * ds + r.len);
    }
}

typedef std::tuple<uint64_t, uint64_t, int64_t> Piece;      // source address, destination address, bytes

// the views of the list, checked against their definition -> the number of views of k > 1
static int64_t check_views(const std::vector<xg_vrow> &rows, int64_t tb, int tp)
{
    const int64_t n = (int64_t)rows.size();
    std::vector<int64_t> order((size_t)n + 1, -1);
    std::vector<int32_t> k((size_t)n + 1), kind((size_t)n + 1);
    const int64_t nv = xg_vrow_views(rows.data(), n, tb, tp, order.data(), k.data(), kind.data());
    CHECK(nv >= 0 && nv <= n && xg_vrow_views(rows.data(), n, tb, tp, nullptr, nullptr, nullptr) == nv);
    std::vector<char> seen((size_t)n, 0);
    int64_t at = 0, multi = 0;
    for (int64_t v = 0; v < nv; ++v) {
        CHECK(k[(size_t)v] >= 1 && at + k[(size_t)v] <= n);
        const xg_vrow &f = rows[(size_t)order[(size_t)at]];
        CHECK((k[(size_t)v] > 1) == (kind[(size_t)v] != XG_VIEW_SINGLE));
        if (k[(size_t)v] > 1) {
            CHECK(f.len <= tb && k[(size_t)v] <= tp && k[(size_t)v] * f.len <= tb);
            ++multi;
        }
        for (int i = 0; i < k[(size_t)v]; ++i) {
            const int64_t idx = order[(size_t)(at + i)];
            CHECK(idx >= 0 && idx < n && !seen[(size_t)idx]);
            seen[(size_t)idx] = 1;
            const xg_vrow &r = rows[(size_t)idx];
            CHECK(r.src_buf == f.src_buf && r.dst_buf == f.dst_buf && r.len == f.len && r.count == f.count &&
                  r.src_step == f.src_step && r.dst_step == f.dst_step);
            if (kind[(size_t)v] == XG_VIEW_DST_STRIPED) CHECK(r.dst_off == f.dst_off + i * f.len);
            if (kind[(size_t)v] == XG_VIEW_SRC_STRIPED) CHECK(r.src_off == f.src_off + i * f.len);
        }
        at += k[(size_t)v];
    }
    CHECK(at == n);
    return multi;
}

// walk == false: only the cut rule (a launch too large to walk)
static void check_launch(const std::vector<xg_vrow> &rows, int64_t tb, int tp, int64_t cap, bool walk, int64_t want_multi = -1)
{
    uint64_t base[XG_NBUF];
    int64_t bytes[XG_NBUF];
    regions_of(rows, base, bytes);
    const int64_t multi = check_views(rows, tb, tp);
    if (want_multi >= 0) CHECK(multi == want_multi);
    xg_view_tables *t = nullptr;
    CHECK(xg_view_tables_build(rows.data(), (int64_t)rows.size(), base, bytes, tb, tp, cap, &t) == XG_OK && t);
    const int64_t T = xg_view_tables_tiles(t), B = xg_view_tables_bytes(t);
    const int nd = xg_view_tables_dispatches(t);
    CHECK(xg_view_tables_multi(t) == multi && xg_view_tables_rows(t) == (int64_t)rows.size());
    CHECK((int64_t)t->tile0.size() == xg_view_tables_views(t) + 1 && t->tile0[0] == 0 && t->tile0.back() == T);
    CHECK(xg_view_tables_cut(t, 0) == 0 && xg_view_tables_cut(t, nd) == T && xg_view_tables_cut(t, nd + 1) == -1);
    CHECK(xg_view_tables_order(t, -1) == -1 && xg_view_tables_order(t, (int64_t)rows.size()) == -1);
    if (cap == 0 || B <= cap + cap / 2) CHECK(nd == (T > 0));
    int64_t sum = 0;
    for (int d = 0; d < nd; ++d) {
        const int64_t b = xg_view_tables_cut(t, d), e = xg_view_tables_cut(t, d + 1), nb = xg_view_tables_dispatch_bytes(t, d);
        CHECK(b < e && nb > 0);
        if (d + 1 < nd) CHECK(nb >= cap);
        else if (nd > 1) CHECK(e - b >= 16 && nb >= cap / 2);
        sum += nb;
    }
    CHECK(sum == B);
    int64_t row0 = 0;
    for (size_t v = 0; v < t->views.size(); ++v) {
        CHECK(t->views[v].row0 == row0 && t->views[v].k >= 1 && t->views[v].jb >= 1 && t->tile0[v] < t->tile0[v + 1]);
        row0 += t->views[v].k;
    }
    CHECK(row0 == (int64_t)rows.size());
    if (walk) {
        // what the rows mean: every block, cut at the tile size
        std::map<Piece, int> want;
        for (const xg_vrow &x : rows) {
            const int64_t ss = x.count > 1 ? x.src_step : 0, ds = x.count > 1 ? x.dst_step : 0;
            for (int64_t j = 0; j < x.count; ++j)
                for (int64_t o = 0; o < x.len; o += tb)
                    ++want[Piece(base[x.src_buf] + (uint64_t)(x.src_off + j * ss + o),
                                 base[x.dst_buf] + (uint64_t)(x.dst_off + j * ds + o), std::min(tb, x.len - o))];
        }
        // every lane of every tile of every dispatch, as the kernel derives it
        for (int d = 0; d < nd; ++d) {
            int64_t nb = 0, last = 0;
            for (int64_t tile = xg_view_tables_cut(t, d); tile < xg_view_tables_cut(t, d + 1); ++tile) {
                size_t v = 0;
                while (t->tile0[v + 1] <= tile) ++v;
                const xgk::DView &w = t->views[v];
                const xgk::DVRow &r0 = t->rows[(size_t)w.row0];
                std::vector<xg_vrow> mine;
                for (int i = 0; i < w.k; ++i) mine.push_back(rows[(size_t)t->order[(size_t)(w.row0 + i)]]);
                last = 0;
                uint64_t prev = 0;
                bool idle = false;
                for (int lane = 0; lane < xgk::kThreads; ++lane) {
                    const xg_view_at p = xg_view_piece_at(r0.len, r0.count, w.k, w.jb, tb, tile - t->tile0[v], lane);
                    if (lane < tp) {
                        int row = -1;
                        int64_t so = -1, dof = -1, pn = -1;
                        CHECK(xg_view_piece(mine.data(), w.k, tb, tp, tile - t->tile0[v], lane, &row, &so, &dof, &pn) == 0);
                        CHECK(row == p.row && pn == p.n);
                        if (pn) CHECK(so == mine[(size_t)row].src_off + p.block * r0.src_step + p.off &&
                                      dof == mine[(size_t)row].dst_off + p.block * r0.dst_step + p.off);
                    }
                    if (!p.n) {
                        idle = true;
                        continue;
                    }
                    CHECK(!idle && lane < tp && p.row >= 0 && p.row < w.k && p.row == lane % w.k);
                    const xgk::DVRow &r = t->rows[(size_t)(w.row0 + p.row)];
                    const uint64_t s = (uint64_t)(uintptr_t)r.src + (uint64_t)(p.block * r0.src_step + p.off);
                    const uint64_t dd = (uint64_t)(uintptr_t)r.dst + (uint64_t)(p.block * r0.dst_step + p.off);
                    auto it = want.find(Piece(s, dd, p.n));
                    CHECK(it != want.end() && it->second > 0);
                    --it->second;
                    // across the rows of a dst-striped view the tile's destinations ascend, len apart
                    if (t->kind[v] == XG_VIEW_DST_STRIPED && p.row > 0) CHECK(dd == prev + (uint64_t)r0.len);
                    prev = dd;
                    nb += p.n; last += p.n;
                }
                CHECK(last > 0);
            }
            CHECK(nb == xg_view_tables_dispatch_bytes(t, d));
            if (d + 1 < nd) CHECK(nb < cap + last);         // at most one tile over the cap
        }
        for (const auto &kv : want) CHECK(kv.second == 0);
    }
    const int64_t n = xg_view_tables_dump(t, nullptr, 0);
    std::vector<char> text((size_t)n + 1);
    CHECK(xg_view_tables_dump(t, text.data(), n + 1) == n && text[n] == 0);
    xg_view_tables_free(t);
    ++g_launches;
}

static void check_refused(xg_vrow r, int64_t region)
{
    uint64_t base[XG_NBUF] = {1ull << 44, 2ull << 44, 0, 0, 0};
    int64_t bytes[XG_NBUF] = {region, region, 0, 0, 0};
    xg_view_tables *t = (xg_view_tables *)1;
    CHECK(xg_view_tables_build(&r, 1, base, bytes, 32768, 256, 0, &t) == XG_EARG && t == nullptr);
    const xg_vrow two[2] = {{XG_BUF_SEND, XG_BUF_RECV, 0, 0, 8, 8, 8, 2}, r};
    t = (xg_view_tables *)1;
    CHECK(xg_view_tables_build(two, 2, base, bytes, 32768, 256, 0, &t) == XG_EARG && t == nullptr);
}

// k rows of one dst-striped view: the destinations n apart with `gap` bytes between strides
static std::vector<xg_vrow> view_rows(int k, int64_t n, int64_t count, int64_t gap, int64_t src0, int64_t dst0)
{
    std::vector<xg_vrow> out;
    for (int i = 0; i < k; ++i)
        out.push_back({XG_BUF_SEND, XG_BUF_RECV, src0 + i * (count * n + 3), dst0 + i * n, n, k * n + gap, n, count});
    return out;
}

int main()
{
    static const int64_t tbs[] = {32768, 64};
    static const int tps[] = {256, 1, 5};
    const int S = XG_BUF_SEND, R = XG_BUF_RECV;
    // the deal: k x len, a count that leaves the last tile partial
    for (int k : {1, 2, 3, 5, 16, 17, 255, 256})
        for (int64_t n : {1, 7, 16, 17, 64, 100, 1000}) {
            if (k > std::min<int64_t>(256, std::max<int64_t>(1, 32768 / n))) continue;
            const int64_t jb = xg_view_jb(n, k, 32768, 256);
            snprintf(g_what, sizeof g_what, "deal k %d len %lld", k, (long long)n);
            CHECK(jb >= 1 && jb * k <= 256 && (jb * k * n <= 32768 || jb == 1));
            check_launch(view_rows(k, n, 2 * jb + (jb + 1) / 2, 0, 7, 11), 32768, 256, 0, true, k > 1);
            check_launch(view_rows(k, n, 2 * jb + (jb + 1) / 2, 5, 7, 11), 32768, 256, 3000, true, k > 1);
        }
    // hand-made rows that are no views, a view among them, in list order and reversed
    std::vector<xg_vrow> hand = {
        {S, R, 0, 3, 16, 37, 16, 700},          {S, R, 11200, 30000, 1000, 1003, 1000, 40},
        {S, R, 52000, 80000, 0, 0, 1, 1},       {S, R, 52001, 80001, 32768, 32771, 32768, 2},
        {S, R, 120000, 150000, 32784, 32784, 32784, 2}, {S, R, 190000, 220000, 100000, 100001, 100000, 3},
        {S, R, 500000, 530000, 65, 65, 65, 129},
        {S, R, 600000, 700000, 4099, ((int64_t)1 << 31) + 48, 4096, 3},      // block offsets past 2^31
        {S, R, 700000, 800000, ((int64_t)1 << 32) + 16, 4101, 4096, 2},
    };
    for (const xg_vrow &r : view_rows(5, 48, 300, 5, ((int64_t)1 << 33) + 1, ((int64_t)1 << 34) + 9)) hand.push_back(r);
    // a view whose steps pass 2^31
    hand.push_back({S, R, ((int64_t)1 << 35), ((int64_t)1 << 36) + 3, ((int64_t)1 << 31) + 49, ((int64_t)1 << 31) + 48, 4096, 5});
    hand.push_back({S, R, ((int64_t)1 << 35) + 9000, ((int64_t)1 << 36) + 3 + 4096, ((int64_t)1 << 31) + 49, ((int64_t)1 << 31) + 48, 4096, 5});
    std::vector<xg_vrow> reversed(hand.rbegin(), hand.rend());
    for (int64_t tb : tbs)
        for (int tp : tps)
            for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)700, (int64_t)4096, (int64_t)65536, (int64_t)1 << 40}) {
                snprintf(g_what, sizeof g_what, "hand tb %lld tp %d cap %lld", (long long)tb, tp, (long long)cap);
                check_launch(hand, tb, tp, cap, true, tb == 32768 && tp >= 5 ? 2 : -1);
                check_launch(reversed, tb, tp, cap, true);
            }
    // long chains: 257 rows of 16 B are 256 + 1, 40 rows of 1000 B are 32 + 8
    snprintf(g_what, sizeof g_what, "long chains");
    {
        std::vector<xg_vrow> rows = view_rows(257, 16, 4, 0, 0, 0);
        std::vector<int32_t> k(257);
        CHECK(xg_vrow_views(rows.data(), 257, 32768, 256, nullptr, k.data(), nullptr) == 2 && k[0] == 256 && k[1] == 1);
        check_launch(rows, 32768, 256, 0, true, 1);
        rows = view_rows(40, 1000, 4, 0, 0, 0);
        CHECK(xg_vrow_views(rows.data(), 40, 32768, 256, nullptr, k.data(), nullptr) == 2 && k[0] == 32 && k[1] == 8);
        check_launch(rows, 32768, 256, 0, true, 2);
        rows = view_rows(3, 32768 + 16, 2, 0, 0, 0);
        check_launch(rows, 32768, 256, 0, true, 0);
    }
    // a striped domain through the schedule: xg_vec_rows_build's rows on 1 and 2 GPUs, both directions
    {
        const int P = 6, A = 3;
        int rl[A];
        xg_aggregator_list(P, A, 1, 1, rl);
        for (int64_t L : {64, 100}) {
            std::vector<xg_vec> v;
            int64_t dom[A];
            for (int r = 0; r < P; ++r)                 // rank-major: an aggregator's rows are A apart
                for (int a = 0; a < A; ++a) v.push_back({r, a, r * L, L, P * L, 37 + a});
            for (int a = 0; a < A; ++a) {
                v.push_back({a, a, P * L * 40, 40000, 0, 1});
                dom[a] = P * L * 40 + 40000 + a;
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
                        for (int64_t cap : {(int64_t)0, (int64_t)1000, (int64_t)30000}) {
                            snprintf(g_what, sizeof g_what, "vecs L %lld m %d G %d g %d cap %lld", (long long)L, m, G, g,
                                     (long long)cap);
                            check_launch(rows, 32768, 256, cap, true, G == 1 ? A : -1);
                            check_launch(rows, 64, 5, cap, true);
                        }
                    }
                xg_sched_free(s);
            }
        }
    }
    // the states of the cutting rule inside a view; 2^30 blocks
    {
        const int64_t T16 = 128 * 128;      // a tile of a view of 2 rows of 64-B blocks: jb 128
        snprintf(g_what, sizeof g_what, "cut states");
        for (int64_t tiles : {148, 96, 97})
            check_launch(view_rows(2, 64, 128 * tiles, 0, 0, 0), 32768, 256, 64 * T16, true, 1);
        check_launch(view_rows(2, 16, (int64_t)1 << 30, 0, 0, 0), 32768, 256, (int64_t)512 << 20, false, 1);
        check_launch(view_rows(2, 16, (int64_t)1 << 29, 0, 0, 0), 64, 2, (int64_t)512 << 20, false, 1);
        check_launch({}, 32768, 256, 4096, true, 0);
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
        uint64_t base[XG_NBUF] = {1ull << 44, 2ull << 44, 0, 0, 0};
        int64_t bytes[XG_NBUF] = {big, big, 0, 0, 0};
        const xg_vrow ok = {S, R, 0, 0, 8, 8, 8, 2};
        xg_view_tables *t = nullptr;
        CHECK(xg_view_tables_build(&ok, 1, base, bytes, 0, 256, 0, &t) == XG_EARG);
        CHECK(xg_view_tables_build(&ok, 1, base, bytes, 32768, 257, 0, &t) == XG_EARG);
        CHECK(xg_view_tables_build(&ok, 1, base, bytes, 32768, 256, -1, &t) == XG_EARG);
        CHECK(xg_vrow_views(&ok, 1, 0, 256, nullptr, nullptr, nullptr) == -1);
        CHECK(xg_view_piece(&ok, 1, 32768, 256, 1, 0, nullptr, nullptr, nullptr, nullptr) == -1);
        CHECK(xg_view_piece(&ok, 1, 32768, 256, 0, 256, nullptr, nullptr, nullptr, nullptr) == -1);
        CHECK(xg_view_piece(&ok, 1, 32768, 256, 0, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    }
    printf("%d launches covered\n", g_launches);
    return g_launches > 150 ? 0 : 1;
}
