// plan_tables_san.cc -- a stand-alone program for the sanitizers (test_plan_tables.py compiles it with
// csrc/host/plan_tables.cc and the C host sources under -fsanitize=address,undefined and runs it):
// builds the plan tables of a handful of device plans and checks, in C++ over the tables
// themselves, that every positive copy is covered exactly once by the pieces and rows of its step's
// launches (or, deferred, of the next step's launch that holds the previous unpacks).  It also drives
// the knobs' environment parser (xg_plan_knobs_env) with scripted arrays.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "plan_tables.h"

#define CHECK(x)                                                                    \
    do {                                                                            \
        if (!(x)) {                                                                 \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #x, g_what); \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

static char g_what[256];
static int g_plans = 0;

typedef std::tuple<uint64_t, uint64_t> Key;        // (source address, destination address)

static void check_cover(const xg_devplan *dp, const PlanKnobs *k)
{
    uint64_t base[XG_NBUF];
    int64_t bytes[XG_NBUF];
    for (int b = 0; b < XG_NBUF; ++b) {
        base[b] = (uint64_t)(b + 1) << 40;
        bytes[b] = dp->region_bytes[b];
    }
    xg_plan_tables *t = nullptr;
    CHECK(xg_plan_tables_build(dp, k, base, bytes, &t) == XG_OK && t);
    // the pieces as the device scan leaves them
    std::vector<xgk::DCopy> pc = t->pieces;
    for (const xgk::DFix &f : t->ds.fix) {
        CHECK(f.piece >= 0 && f.piece < (int)pc.size() && f.copy >= 0 && f.copy < (int)t->ds.len.size());
        CHECK(f.off + pc[f.piece].len <= t->ds.len[f.copy]);
        if (f.side == 0) pc[f.piece].dst += t->ds.host[f.copy];
        else pc[f.piece].src += t->ds.host[f.copy];
    }
    std::vector<std::multimap<Key, int64_t>> offer(t->launches.size());
    size_t total = 0;
    for (size_t i = 0; i < t->launches.size(); ++i) {
        const CopyLaunch &l = t->launches[i];
        for (int j = l.b; j < l.b + l.n; ++j)
            offer[i].insert({Key((uint64_t)(uintptr_t)pc[j].src, (uint64_t)(uintptr_t)pc[j].dst), pc[j].len});
        if (l.kind == XG_COPY_SMALL)
            for (int j = l.q_row; j < l.q_row + l.q_copies; ++j)
                offer[i].insert({Key((uint64_t)(uintptr_t)t->rows[j].src, (uint64_t)(uintptr_t)t->rows[j].dst),
                                 t->rows[j].len});
        total += offer[i].size();
        // the dispatches tile the launch
        const int first = l.kind == XG_COPY_SMALL ? 0 : l.b;
        CHECK(l.ndisp >= 1 && t->cuts[l.cut] == first);
        for (int d = 0; d < l.ndisp; ++d) CHECK(t->cuts[l.cut + d] < t->cuts[l.cut + d + 1] || l.bytes == 0);
        if (l.kind != XG_COPY_SMALL) CHECK(t->cuts[l.cut + l.ndisp] == l.b + l.n);
    }
    size_t used = 0;
    for (int s = 0; s < dp->nsteps; ++s) {
        const xg_stepplan &sp = dp->steps[s];
        const StepR &st = t->steps[s];
        for (int pass = 0; pass < 2; ++pass) {
            const int b = pass ? sp.post_begin : sp.pre_begin, n = pass ? sp.post_count : sp.pre_count;
            for (int i = 0; i < n; ++i) {
                const xg_copy &c = dp->copies[b + i];
                if (c.len <= 0) continue;
                const bool local = !pass && i >= sp.stage_count && c.dst_buf != XG_BUF_STAGE_SEND;
                if (local && st.self_local) continue;
                int lo = st.l_b, hi = st.l_e;
                if (pass && st.deferred) {
                    CHECK(s + 1 < dp->nsteps);
                    lo = t->steps[s + 1].l_b; hi = t->steps[s + 1].l_e;
                }
                int took = -1;
                for (int64_t o = 0; o < c.len;) {
                    const Key key(base[c.src_buf] + c.src_off + o, base[c.dst_buf] + c.dst_off + o);
                    int found = -1;
                    for (int j = lo; j < hi; ++j)
                        if ((!(pass && st.deferred) || t->launches[j].mark_prev) && offer[j].count(key)) {
                            CHECK(found < 0);
                            found = j;
                        }
                    CHECK(found >= 0 && (took < 0 || took == found));
                    took = found;
                    auto it = offer[found].find(key);
                    CHECK(it->second > 0 && it->second <= c.len - o);
                    o += it->second;
                    offer[found].erase(it);
                    ++used;
                }
            }
        }
    }
    CHECK(used == total);
    // the text dump runs over every table
    const int64_t n = xg_plan_tables_dump(t, nullptr, 0);
    std::vector<char> text((size_t)n + 1);
    CHECK(xg_plan_tables_dump(t, text.data(), n + 1) == n && text[n] == 0);
    xg_plan_tables_free(t);
    ++g_plans;
}

// xg_plan_knobs_env over scripted environments.  Every entry is a heap string of its exact length,
// so a read past an entry's end (a name longer than the entry, an entry without '=') is the
// sanitizer's to find.  -> the number of environments read
static int knob_environments()
{
    snprintf(g_what, sizeof g_what, "knob environments");
    const int nn = xg_plan_knob_names(nullptr, 0);
    std::vector<const char *> names((size_t)nn);
    CHECK(nn > 20 && xg_plan_knob_names(names.data(), nn) == nn);
    const std::string nines(1 << 20, '9');
    std::vector<std::string> all;
    for (const char *n : names) all.push_back(std::string(n) + "=1");
    const std::vector<std::vector<std::string>> envs = {
        {},
        {"XG_SELF_MAX=" + nines, "XG_ENGINE_SOLO=0" + nines, "XG_WAVE_KIB=" + std::string(1 << 20, ' ') + "8"},
        {"XG_ENGINE_WG=99999999999", "XG_SOLO_RAILS=99999999999", "XG_SMALL_PIECE_ORDER=4294967297",
         "XG_EXTENT_TILE_KIB=4294967297", "XG_SPLIT_MIN=99999999999"},
        {"XG_SELF_MAX", "XG_SELF_MA", "X", "", "XG_SELF_MAX=3"},
        {"=5", "==", "=XG_SELF_MAX=4", "XG_SELF_MAX=6"},
        all,
        {"XG_STEP_CHAIN=0", "XG_STEP_CHAIN=1", "XG_SELF_MAX=7", "XG_SELF_MAX=8"},
        {"XG_COPY_CHUNK=1", "XG_COPY_VARIANT=0"},                 // a retired name: one line on stderr
    };
    int read = 0;
    for (const auto &e : envs) {
        std::vector<char *> arr;
        for (const std::string &s : e) arr.push_back(strdup(s.c_str()));
        arr.push_back(nullptr);
        xg_plan_knobs k, d;
        xg_plan_knobs_default(&k, 256, 256, 2048);
        xg_plan_knobs_default(&d, 256, 256, 2048);
        xg_plan_knobs_env(&k, arr.data());
        for (char *s : arr) free(s);
        CHECK(k.engine_wmax >= 1 && k.engine_wmax <= 256 && k.solo_rails >= 1 && k.solo_rails <= XG_SOLO_MAX_RAILS);
        CHECK(k.rules.small_order >= 1 && k.rules.small_order <= 1024 && k.extent_tile >= 1024 && k.extent_tile <= 1 << 20);
        switch (read) {
        case 0: CHECK(!memcmp(&k, &d, sizeof k)); break;
        case 1: CHECK(k.self_max == INT64_MAX && k.solo == 1 && k.rules.wave_kib == 8); break;
        case 2: CHECK(k.split_min == 99999999999ll); break;
        case 3: CHECK(k.self_max == 3); break;
        case 4: CHECK(k.self_max == 6); break;
        case 5: CHECK(k.variant == 1 && k.engine_wmax == 1 && k.wave_grid == 1 && k.solo_rails == 1 && k.self_max == 1 &&
                      k.extent_tile == 1024 && k.engine_drain == 1 && k.engine_arm == 1 && k.rules.wave_kib == 0); break;
        case 6: CHECK(k.step_chain == 0 && k.self_max == 7); break;
        default: CHECK(!memcmp(&k, &d, sizeof k)); break;
        }
        ++read;
    }
    return read;
}

int main()
{
    PlanKnobs k;
    static const int64_t caps[] = {512 << 20, 4096, 1, 0};
    // uniform schedules: P 16, A 5, -d 4096 (methods of every kind, TAM included) on 1, 2 and 8 GPUs, direct and
    // in every pack form
    const int P = 16, A = 5;
    int rl[A];
    CHECK(xg_aggregator_list(P, A, 1, 1, rl) == 0 || true);
    char err[256];
    static const int methods[] = {1, 2, 4, 6, 9, 12, 15, 16, 18};
    for (int m : methods) {
        xg_sched *s = xg_sched_build(m, P, A, 4096, 3, rl, 2, 4, 0, 65424, err, sizeof err);
        snprintf(g_what, sizeof g_what, "method %d", m);
        CHECK(s);
        for (int G : {1, 2, 8})
            for (int form = -1; form <= 3; ++form) {
                if (G == 1 && form >= 0) continue;
                for (int g = 0; g < G; ++g) {
                    xg_devplan *dp = xg_devplan_build_form(s, G, g, form < 0 ? 0 : 4 << 20, 0, form);
                    if (!dp) continue;          // a form the method does not take
                    for (int64_t cap : caps) {
                        xg_plan_knobs_default(&k, 256, 256, 2048);
                        k.rank = g; k.nranks = G; k.virt = G > 1; k.launch_max = cap;
                        snprintf(g_what, sizeof g_what, "method %d G %d g %d form %d cap %lld", m, G, g, form,
                                 (long long)cap);
                        check_cover(dp, &k);
                    }
                    xg_devplan_free(dp);
                }
            }
        xg_sched_free(s);
    }
    // a ragged schedule (lengths off the 16-B grid, some empty) and its placement plan
    {
        const int p = 7, a = 3;
        int rl2[a];
        xg_aggregator_list(p, a, 1, 1, rl2);
        int64_t lens[p * a];
        std::vector<xg_ext> exts;
        int64_t dom[a] = {0, 0, 0};
        for (int r = 0; r < p; ++r)
            for (int j = 0; j < a; ++j) {
                lens[r * a + j] = (r * 7 + j * 13) % 5 == 0 ? 0 : 1000 + 37 * r + 411 * j;
                for (int64_t left = lens[r * a + j], e = 0; left > 0; ++e) {      // extents of 1..300 B with gaps
                    const int64_t n = std::min<int64_t>(left, 1 + (r * 31 + j * 17 + e * 7) % 300);
                    exts.push_back({r, j, dom[j] + (e % 3) * 5, n});
                    dom[j] += (e % 3) * 5 + n;
                    left -= n;
                }
            }
        for (int m : {1, 2}) {
            xg_sched *s = xg_sched_build_v(m, p, a, lens, 2, rl2, 1, 1, 0, 65424, 0, err, sizeof err);
            snprintf(g_what, sizeof g_what, "ragged method %d", m);
            CHECK(s);
            for (int G : {1, 2})
                for (int g = 0; g < G; ++g) {
                    xg_devplan *plans[2] = {xg_devplan_build_form(s, G, g, G > 1 ? 1 << 20 : 0, 0, -1),
                                            xg_place_plan_build(s, G, g, exts.data(), (int64_t)exts.size(), dom)};
                    for (xg_devplan *dp : plans) {
                        CHECK(dp);
                        for (int64_t cap : caps) {
                            xg_plan_knobs_default(&k, 256, 256, 2048);
                            k.rank = g; k.nranks = G; k.virt = G > 1; k.launch_max = cap;
                            check_cover(dp, &k);
                        }
                        xg_devplan_free(dp);
                    }
                }
            xg_sched_free(s);
        }
    }
    printf("knob environments: %d read\n", knob_environments());
    printf("%d plans covered\n", g_plans);
    return g_plans > 100 ? 0 : 1;
}
