/*
 * agree_check.c -- TEST INFRASTRUCTURE ONLY: csrc/host/agree.h against a scripted peer
 * (tests/test_agree.py builds and runs it; one line per case on stdout).  xg_allreduce_max here
 * records what was posted and answers with the element-wise MAX of it and the peer's vector, or
 * with an error code.
 */
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "agree.h"

static double g_peer[8], g_posted[8];
static int g_fail, g_n;

int xg_allreduce_max(xg_ctx *ctx, double *vals, int n)
{
    int i;
    (void)ctx;
    g_n = n;
    for (i = 0; i < n && i < 8; ++i) g_posted[i] = vals[i];
    if (g_fail) return g_fail;
    for (i = 0; i < n && i < 8; ++i)
        if (g_peer[i] > vals[i]) vals[i] = g_peer[i];
    return XG_OK;
}

static void script(int fail, double failed, double code, double flag)
{
    memset(g_peer, 0, sizeof g_peer);
    g_peer[0] = failed; g_peer[1] = code; g_peer[2] = flag;
    g_fail = fail;
    g_n = -1;
}

static void peers(int local, int peer_code, int fail)
{
    char err[128] = "untouched";
    int rc;
    script(fail, peer_code ? 1.0 : 0.0, peer_code, 0.0);
    rc = agree_peers(NULL, local, NULL, "doing this", err, sizeof err);
    printf("peers local=%d peer=%d allreduce=%d -> rc=%d posted=%d (%g %g) err=[%s]\n", local, peer_code, fail, rc, g_n,
           g_posted[0], g_posted[1], err);
}

static void route(int local, int flag, int peer_flag)
{
    char err[128] = "untouched";
    int f = flag, rc;
    script(0, 0.0, 0.0, peer_flag);
    rc = agree_peers(NULL, local, &f, "doing this", err, sizeof err);
    printf("route local=%d flag=%d peer=%d -> rc=%d flag=%d posted=%d (%g) err=[%s]\n", local, flag, peer_flag, rc, f, g_n,
           g_posted[2], err);
}

/* the peer's digest is h with `delta` added to 16-bit part `part` (delta 0: the same digest) */
static void digest(uint64_t h, int part, int delta, int fail)
{
    int j, differ = -1, rc, mirrored = 1;
    script(fail, 0.0, 0.0, 0.0);
    for (j = 0; j < 4; ++j) {
        g_peer[j] = (double)((h >> (16 * j)) & 0xffff) + (j == part ? delta : 0);
        g_peer[4 + j] = -g_peer[j];
    }
    rc = agree_digest(NULL, h, &differ);
    for (j = 0; j < 4; ++j) mirrored &= g_posted[j] == (double)((h >> (16 * j)) & 0xffff) && g_posted[4 + j] == -g_posted[j];
    printf("digest part=%d delta=%d allreduce=%d -> rc=%d differ=%d posted=%d mirrored=%d\n", part, delta, fail, rc, differ,
           g_n, mirrored);
}

int main(void)
{
    const uint64_t h = 0x0123456789abcdefull;   /* no part is 0 or 0xffff: part +- 1 stays a 16-bit part */
    int part;
    peers(0, 0, 0);
    peers(4, 0, 0);
    peers(0, 4, 0);
    peers(2, 4, 0);
    peers(0, 0, 7);
    peers(4, 0, 7);
    route(0, 0, 1);
    route(0, 1, 0);
    route(0, 0, 0);
    route(4, 0, 1);
    digest(h, 0, 0, 0);
    for (part = 0; part < 4; ++part) {
        digest(h, part, +1, 0);
        digest(h, part, -1, 0);
    }
    digest(h, 0, 0, 7);
    printf("fnv \"\" = %016" PRIx64 "\n", agree_fnv(AGREE_FNV_INIT, "", 0));
    printf("fnv \"a\" = %016" PRIx64 "\n", agree_fnv(AGREE_FNV_INIT, "a", 1));
    return 0;
}
