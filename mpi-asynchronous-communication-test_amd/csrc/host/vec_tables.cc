// vec_tables.cc -- the host tables of a row launch (xg_sched.h, "row launch tables"): GPU g's
// xg_vrow list turned into everything one copy_kernel_v launch reads -- the device rows (absolute
// pointers), tile0 (the prefix of the rows' tile counts) and the dispatch cuts.  Everything a load
// decides is decided here, in code that runs, is tested and is sanitized without a GPU; the runtime
// (csrc/runtime/vecplace.hip) only uploads what this file made and walks the finished cut table.
// The second half does the same for a view launch (xg_view_tables_build: copy_kernel_vv, one
// workgroup per tile of one striped view): the views are xg_vrow_views' (vecs.c), the row checks
// and the dispatch cutter are the ones above.
#include "vec_tables.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>

namespace {

// the tile arithmetic of one row, in closed form: O(1) whatever its count
struct RowTiles {
    int64_t len, count, tile_bytes;
    int64_t bpt;        // blocks per tile (len <= tile_bytes), else 0
    int64_t ppb;        // pieces (= tiles) per block (len > tile_bytes), else 0
    int64_t nt;         // its tiles
    RowTiles(const xgk::DVRow &r, int64_t tb, int tp) : len(r.len), count(r.count), tile_bytes(tb), bpt(0), ppb(0)
    {
        if (len <= tb) bpt = xg_vec_bpt(len, tb, tp);
        else ppb = len / tb + (len % tb != 0);
        nt = xg_vec_row_tiles(len, count, tb, tp);
    }
    // a view of k rows of short blocks (k x len <= tb): a row of blocks of k x len bytes, jb to a tile
    RowTiles(const xgk::DVRow &r, int k, int64_t jb, int64_t tb)
        : len(k * r.len), count(r.count), tile_bytes(tb), bpt(jb), ppb(0), nt(r.count / jb + (r.count % jb != 0))
    {
    }
    // the bytes of the row's tiles [0, t), t in [0, nt]
    int64_t before(int64_t t) const
    {
        if (bpt) return std::min(t * bpt, count) * len;             // whole blocks; the last tile holds fewer
        return (t / ppb) * len + (t % ppb) * tile_bytes;            // (t % ppb) * tile_bytes < len: only a block's
    }                                                               // last piece is short
    // the first tile e in (a, nt] with before(e) - before(a) >= need (need > 0), or nt when the
    // row's tiles from a hold less
    int64_t reach(int64_t a, int64_t need) const
    {
        if (before(nt) - before(a) < need) return nt;
        if (bpt) return std::min(nt, a + (need + bpt * len - 1) / (bpt * len));
        const int64_t target = before(a) + need, j = target / len, rem = target - j * len;
        return j * ppb + (rem + tile_bytes - 1) / tile_bytes;       // rem < len: at most ppb pieces
    }
};

bool refuse(const char *who, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
bool refuse(const char *who, const char *fmt, ...)
{
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    fprintf(stderr, "%s: %s\n", who, line);
    return false;
}

// block 0 and block count - 1 of one side of a row inside its region, in 64 bits: every product and
// sum is checked, so an offset that wraps is refused and never compared
bool side_inside(const char *who, int64_t k, const char *side, int buf, int64_t off, int64_t step, int64_t len, int64_t count,
                 const int64_t *bytes)
{
    if (buf < 0 || buf >= XG_NBUF) return refuse(who, "row %lld: %s region %d is none", (long long)k, side, buf);
    int64_t span, last, end;
    if (__builtin_mul_overflow(count - 1, step, &span) || __builtin_add_overflow(off, span, &last) ||
        __builtin_add_overflow(last, len, &end) || __builtin_add_overflow(off, len, &end))
        return refuse(who, "row %lld: %s offset %lld + %lld x %lld + %lld overflows int64", (long long)k, side, (long long)off,
                      (long long)(count - 1), (long long)step, (long long)len);
    if (off < 0 || off + len > bytes[buf] || last < 0 || last + len > bytes[buf])
        return refuse(who, "row %lld: %s blocks [%lld, +%lld) .. [%lld, +%lld) leave region %d of %lld bytes", (long long)k, side,
                      (long long)off, (long long)len, (long long)last, (long long)len, buf, (long long)bytes[buf]);
    return true;
}

const char *const kVecWho = "xg_vec_tables_build", *const kViewWho = "xg_view_tables_build";

// row k of the list: positive, both sides inside their regions; its bytes join *total
bool check_row(const char *who, int64_t k, const xg_vrow &r, const int64_t *bytes, int64_t *total)
{
    if (r.len <= 0 || r.count <= 0)
        return refuse(who, "row %lld: len %lld, count %lld (both must be positive)", (long long)k, (long long)r.len,
                      (long long)r.count);
    if (!side_inside(who, k, "source", r.src_buf, r.src_off, r.src_step, r.len, r.count, bytes) ||
        !side_inside(who, k, "destination", r.dst_buf, r.dst_off, r.dst_step, r.len, r.count, bytes))
        return false;
    int64_t nb;
    if (__builtin_mul_overflow(r.len, r.count, &nb) || __builtin_add_overflow(*total, nb, total))
        return refuse(who, "row %lld: the launch's bytes overflow int64", (long long)k);
    return true;
}

xgk::DVRow device_row(const xg_vrow &r, const uint64_t *base)
{
    xgk::DVRow d;
    d.src = (const uint8_t *)(uintptr_t)(base[r.src_buf] + (uint64_t)r.src_off);
    d.dst = (uint8_t *)(uintptr_t)(base[r.dst_buf] + (uint64_t)r.dst_off);
    d.src_step = r.count > 1 ? r.src_step : 0;
    d.dst_step = r.count > 1 ? r.dst_step : 0;
    d.len = r.len;
    d.count = r.count;
    return d;
}

bool build_rows(VecTables *t, const xg_vrow *rows, int64_t n)
{
    t->rows.resize((size_t)n);
    t->tile0.assign((size_t)n + 1, 0);
    int64_t tiles = 0, total = 0;
    for (int64_t k = 0; k < n; ++k) {
        const xg_vrow &r = rows[k];
        if (!check_row(kVecWho, k, r, t->bytes, &total)) return false;
        const int64_t nt = xg_vec_row_tiles(r.len, r.count, t->tile_bytes, t->tile_pieces);
        if (nt > INT32_MAX - tiles)
            return refuse(kVecWho, "row %lld: more than %d tiles in one launch", (long long)k, INT32_MAX);
        tiles += nt;
        t->tile0[(size_t)k + 1] = (int32_t)tiles;
        t->rows[(size_t)k] = device_row(r, t->base);
    }
    t->total = total;
    return true;
}

// The views of the list, the rows permuted into their order, a record and a tile count per view.
bool build_views(ViewTables *t, const xg_vrow *rows, int64_t n)
{
    int64_t total = 0;
    for (int64_t k = 0; k < n; ++k)
        if (!check_row(kViewWho, k, rows[k], t->bytes, &total)) return false;
    t->total = total;
    t->order.assign((size_t)n, 0);
    std::vector<int32_t> view_k((size_t)n + 1);
    t->kind.assign((size_t)n + 1, 0);
    const int64_t nv = xg_vrow_views(rows, n, t->tile_bytes, t->tile_pieces, t->order.data(), view_k.data(), t->kind.data());
    if (nv < 0) throw std::bad_alloc();
    t->kind.resize((size_t)nv);
    t->rows.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) t->rows[(size_t)i] = device_row(rows[t->order[(size_t)i]], t->base);
    t->views.resize((size_t)nv);
    t->tile0.assign((size_t)nv + 1, 0);
    int64_t tiles = 0, row0 = 0;
    for (int64_t v = 0; v < nv; ++v) {
        const xgk::DVRow &r = t->rows[(size_t)row0];
        const int k = view_k[(size_t)v];
        const int64_t nt = xg_view_tiles(r.len, r.count, k, t->tile_bytes, t->tile_pieces);
        if (nt > INT32_MAX - tiles)
            return refuse(kViewWho, "row %lld: more than %d tiles in one launch", (long long)t->order[(size_t)row0],
                          INT32_MAX);
        tiles += nt;
        t->tile0[(size_t)v + 1] = (int32_t)tiles;
        t->views[(size_t)v] = xgk::DView{(int32_t)row0, k,
                                         r.len <= t->tile_bytes ? (int32_t)xg_view_jb(r.len, k, t->tile_bytes, t->tile_pieces) : 1, 0};
        t->multi += k > 1;
        row0 += k;
    }
    return true;
}

// The launch's dispatches.  Cuts are tile indices from 0, as cut_small's are workgroup indices
// (plan_tables.cc): a launch of more than 1.5 x launch_max bytes goes as dispatches of about
// launch_max bytes of whole tiles -- the first tile boundary at least launch_max bytes past the
// previous cut, which may lie inside a row -- and no runt dispatch closes the launch (a remainder of
// fewer than 16 tiles or less than launch_max / 2 bytes joins the dispatch before it).  The bytes
// of a row's tiles are a closed form (RowTiles), so this costs O(rows + cuts): a row is entered
// once, plus once per cut that falls inside it.
// tiles_of(r): the RowTiles of entry r of tile0 -- a row of a row launch, a view of a view launch.
template <class Tables, class F>
void cut_tiles(Tables *t, F tiles_of)
{
    const int64_t cap = t->launch_max, T = t->tile0.back(), B = t->total;
    const size_t n = t->tile0.size() - 1;
    t->cuts.assign(1, 0);
    t->dbytes.clear();
    if (T == 0) return;
    if (cap > 0 && B > cap && B - cap > cap / 2) {
        size_t r = 0;           // the row of tile o, the last cut ...
        int64_t a = 0;          // ... o's index inside it ...
        int64_t done = 0;       // ... and the bytes of tiles [0, o)
        // VARIANT: every iteration either pushes a cut e with last cut < e < T (e > o because a
        // dispatch of need > 0 bytes takes at least one tile of row r, or runs on into later rows),
        // or leaves the loop: it does so whenever the next boundary is the launch's end, be it
        // because fewer than cap bytes are left or because what would be left behind e is a runt.
        // Nothing else is a way round: there is no path that keeps o where it was.
        for (;;) {
            int64_t acc = 0;    // bytes of tiles [o, (r, a))
            int64_t e = T;
            while (r < n) {
                const RowTiles rt = tiles_of(r);
                const int64_t left = rt.before(rt.nt) - rt.before(a);
                if (acc + left < cap) {         // the whole rest of the row, and on
                    acc += left;
                    ++r;
                    a = 0;
                    continue;
                }
                const int64_t x = rt.reach(a, cap - acc);       // a < x <= nt
                acc += rt.before(x) - rt.before(a);
                e = t->tile0[r] + x;
                a = x;
                if (a == rt.nt) {
                    ++r;
                    a = 0;
                }
                break;
            }
            if (e >= T || T - e < 16 || B - (done + acc) < cap / 2) break;       // the rest is the last dispatch
            t->cuts.push_back((int32_t)e);
            t->dbytes.push_back(acc);
            done += acc;
        }
        t->dbytes.push_back(B - done);
    } else {
        t->dbytes.push_back(B);
    }
    t->cuts.push_back((int32_t)T);
}

struct Dump {
    const uint64_t *base;
    const int64_t *bytes;
    std::string s;
    void f(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
    {
        char line[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(line, sizeof line, fmt, ap);
        va_end(ap);
        s += line;
    }
    // region+offset of an address: the region that holds it
    std::string at(const void *q) const
    {
        const uint64_t a = (uint64_t)(uintptr_t)q;
        char out[64];
        for (int b = 0; b < XG_NBUF; ++b)
            if (bytes[b] > 0 && a >= base[b] && a < base[b] + (uint64_t)bytes[b]) {
                snprintf(out, sizeof out, "%d+%llu", b, (unsigned long long)(a - base[b]));
                return out;
            }
        snprintf(out, sizeof out, "?+%llx", (unsigned long long)a);
        return out;
    }
    // at most cap bytes of the text, NUL included; the text's length
    int64_t out(char *buf, int64_t cap) const
    {
        const int64_t n = (int64_t)s.size();
        if (buf && cap > 0) {
            const int64_t m = std::min(n, cap - 1);
            memcpy(buf, s.data(), (size_t)m);
            buf[m] = 0;
        }
        return n;
    }
};

}  // namespace

extern "C" int xg_vec_tables_build(const xg_vrow *rows, int64_t n, const uint64_t base[XG_NBUF],
                                   const int64_t bytes[XG_NBUF], int64_t tile_bytes, int tile_pieces, int64_t launch_max,
                                   xg_vec_tables **out)
{
    if (out) *out = nullptr;
    if (!out || n < 0 || (n > 0 && !rows) || !base || !bytes || tile_bytes < 1 || tile_pieces < 1 ||
        tile_pieces > xgk::kThreads || launch_max < 0) {
        fprintf(stderr, "xg_vec_tables_build: bad arguments (n %lld, tile_bytes %lld, tile_pieces %d, launch_max %lld)\n",
                (long long)n, (long long)tile_bytes, tile_pieces, (long long)launch_max);
        return XG_EARG;
    }
    VecTables *t = new (std::nothrow) VecTables;
    if (!t) return XG_ENOMEM;
    memcpy(t->base, base, sizeof t->base);
    memcpy(t->bytes, bytes, sizeof t->bytes);
    t->tile_bytes = tile_bytes;
    t->tile_pieces = tile_pieces;
    t->launch_max = launch_max;
    try {
        if (!build_rows(t, rows, n)) {
            delete t;
            return XG_EARG;
        }
        cut_tiles(t, [t](size_t r) { return RowTiles(t->rows[r], t->tile_bytes, t->tile_pieces); });
    } catch (const std::bad_alloc &) {
        delete t;
        return XG_ENOMEM;
    }
    *out = t;
    return XG_OK;
}

extern "C" void xg_vec_tables_free(xg_vec_tables *t) { delete t; }
extern "C" int64_t xg_vec_tables_rows(const xg_vec_tables *t) { return (int64_t)t->rows.size(); }
extern "C" int64_t xg_vec_tables_tiles(const xg_vec_tables *t) { return t->tile0.back(); }
extern "C" int xg_vec_tables_dispatches(const xg_vec_tables *t) { return (int)t->cuts.size() - 1; }
extern "C" int64_t xg_vec_tables_bytes(const xg_vec_tables *t) { return t->total; }

extern "C" int64_t xg_vec_tables_cut(const xg_vec_tables *t, int k)
{
    return k < 0 || k >= (int)t->cuts.size() ? -1 : t->cuts[(size_t)k];
}

extern "C" int64_t xg_vec_tables_dispatch_bytes(const xg_vec_tables *t, int k)
{
    return k < 0 || k >= (int)t->dbytes.size() ? -1 : t->dbytes[(size_t)k];
}

extern "C" int64_t xg_vec_tables_dump(const xg_vec_tables *t, char *buf, int64_t cap)
{
    Dump d{t->base, t->bytes, {}};
    d.f("vec rows %zu tiles %d dispatches %zu bytes %lld tile_bytes %lld tile_pieces %d launch_max %lld\n", t->rows.size(),
        t->tile0.back(), t->cuts.size() - 1, (long long)t->total, (long long)t->tile_bytes, t->tile_pieces,
        (long long)t->launch_max);
    for (size_t i = 0; i < t->rows.size(); ++i) {
        const xgk::DVRow &r = t->rows[i];
        d.f("row %zu %s %s %lld %lld %lld %lld\n", i, d.at(r.src).c_str(), d.at(r.dst).c_str(), (long long)r.src_step,
            (long long)r.dst_step, (long long)r.len, (long long)r.count);
    }
    for (size_t i = 0; i < t->tile0.size(); ++i) d.f("tile0 %zu %d\n", i, t->tile0[i]);
    for (size_t i = 0; i < t->cuts.size(); ++i) d.f("cut %zu %d\n", i, t->cuts[i]);
    for (size_t i = 0; i < t->dbytes.size(); ++i) d.f("dbytes %zu %lld\n", i, (long long)t->dbytes[i]);
    return d.out(buf, cap);
}

// ---------------------------------------------------------------- view launch tables
extern "C" int xg_view_tables_build(const xg_vrow *rows, int64_t n, const uint64_t base[XG_NBUF],
                                    const int64_t bytes[XG_NBUF], int64_t tile_bytes, int tile_pieces, int64_t launch_max,
                                    xg_view_tables **out)
{
    if (out) *out = nullptr;
    if (!out || n < 0 || (n > 0 && !rows) || !base || !bytes || tile_bytes < 1 || tile_pieces < 1 ||
        tile_pieces > xgk::kThreads || launch_max < 0) {
        fprintf(stderr, "xg_view_tables_build: bad arguments (n %lld, tile_bytes %lld, tile_pieces %d, launch_max %lld)\n",
                (long long)n, (long long)tile_bytes, tile_pieces, (long long)launch_max);
        return XG_EARG;
    }
    ViewTables *t = new (std::nothrow) ViewTables;
    if (!t) return XG_ENOMEM;
    memcpy(t->base, base, sizeof t->base);
    memcpy(t->bytes, bytes, sizeof t->bytes);
    t->tile_bytes = tile_bytes;
    t->tile_pieces = tile_pieces;
    t->launch_max = launch_max;
    try {
        if (!build_views(t, rows, n)) {
            delete t;
            return XG_EARG;
        }
        // a view of short blocks is, to the cutter, one row of blocks of k x len bytes, jb to a tile;
        // a long block is a view of its own and keeps its row's arithmetic
        cut_tiles(t, [t](size_t v) {
            const xgk::DView &w = t->views[v];
            const xgk::DVRow &r = t->rows[(size_t)w.row0];
            return r.len <= t->tile_bytes ? RowTiles(r, w.k, w.jb, t->tile_bytes) : RowTiles(r, t->tile_bytes, t->tile_pieces);
        });
    } catch (const std::bad_alloc &) {
        delete t;
        return XG_ENOMEM;
    }
    *out = t;
    return XG_OK;
}

extern "C" void xg_view_tables_free(xg_view_tables *t) { delete t; }
extern "C" int64_t xg_view_tables_rows(const xg_view_tables *t) { return (int64_t)t->rows.size(); }
extern "C" int64_t xg_view_tables_views(const xg_view_tables *t) { return (int64_t)t->views.size(); }
extern "C" int64_t xg_view_tables_multi(const xg_view_tables *t) { return t->multi; }
extern "C" int64_t xg_view_tables_tiles(const xg_view_tables *t) { return t->tile0.back(); }
extern "C" int xg_view_tables_dispatches(const xg_view_tables *t) { return (int)t->cuts.size() - 1; }
extern "C" int64_t xg_view_tables_bytes(const xg_view_tables *t) { return t->total; }

extern "C" int64_t xg_view_tables_cut(const xg_view_tables *t, int k)
{
    return k < 0 || k >= (int)t->cuts.size() ? -1 : t->cuts[(size_t)k];
}

extern "C" int64_t xg_view_tables_dispatch_bytes(const xg_view_tables *t, int k)
{
    return k < 0 || k >= (int)t->dbytes.size() ? -1 : t->dbytes[(size_t)k];
}

extern "C" int64_t xg_view_tables_order(const xg_view_tables *t, int64_t i)
{
    return i < 0 || i >= (int64_t)t->order.size() ? -1 : t->order[(size_t)i];
}

extern "C" int64_t xg_view_tables_dump(const xg_view_tables *t, char *buf, int64_t cap)
{
    Dump d{t->base, t->bytes, {}};
    d.f("views rows %zu views %zu multi %lld tiles %d dispatches %zu bytes %lld tile_bytes %lld tile_pieces %d launch_max %lld\n",
        t->rows.size(), t->views.size(), (long long)t->multi, t->tile0.back(), t->cuts.size() - 1, (long long)t->total,
        (long long)t->tile_bytes, t->tile_pieces, (long long)t->launch_max);
    for (size_t i = 0; i < t->rows.size(); ++i) {
        const xgk::DVRow &r = t->rows[i];
        d.f("row %zu %s %s %lld %lld %lld %lld\n", i, d.at(r.src).c_str(), d.at(r.dst).c_str(), (long long)r.src_step,
            (long long)r.dst_step, (long long)r.len, (long long)r.count);
    }
    for (size_t i = 0; i < t->order.size(); ++i) d.f("order %zu %lld\n", i, (long long)t->order[i]);
    for (size_t i = 0; i < t->views.size(); ++i)
        d.f("view %zu %d %d %d %d\n", i, t->views[i].row0, t->views[i].k, t->views[i].jb, t->kind[i]);
    for (size_t i = 0; i < t->tile0.size(); ++i) d.f("tile0 %zu %d\n", i, t->tile0[i]);
    for (size_t i = 0; i < t->cuts.size(); ++i) d.f("cut %zu %d\n", i, t->cuts[i]);
    for (size_t i = 0; i < t->dbytes.size(); ++i) d.f("dbytes %zu %lld\n", i, (long long)t->dbytes[i]);
    return d.out(buf, cap);
}
