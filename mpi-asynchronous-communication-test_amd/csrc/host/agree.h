/*
 * agree.h -- how the GPU processes of one job agree, the one definition (internal, header-only).
 *
 * Each GPU plans, allocates, fills and loads its part alone, and each derives every GPU's RCCL calls
 * from its own inputs.  Two things must therefore never happen: a rank that planned from other
 * inputs posting calls nobody pairs, and a rank that failed returning while its peers go on to post
 * calls it will never pair -- either way the job hangs inside RCCL.  So
 *   - before anything that could diverge (a schedule refused on one rank only) the ranks compare a
 *     digest of the inputs (agree_fnv, agree_digest): unequal inputs fail alike on every rank;
 *   - after every stretch a rank works through alone, one MAX reduction tells every rank whether any
 *     failed and the highest code (agree_peers): all return an error alike.
 * Both are one xg_allreduce_max of a few doubles; a rank posting one more or one fewer of them than
 * its peers hangs the job as surely, so an operator's sequence of these calls is its wire protocol.
 */
#ifndef XG_AGREE_H
#define XG_AGREE_H

#include <stdio.h>
#include <stdint.h>
#include <stddef.h>

#include "xg.h"

#define AGREE_FNV_INIT 0xcbf29ce484222325ull

/* FNV-1a (64 bit) of n bytes, continued from h */
static inline uint64_t agree_fnv(uint64_t h, const void *p, size_t n)
{
    const unsigned char *b = (const unsigned char *)p;
    size_t i;
    for (i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

/* Whether every rank holds the digest h: one MAX reduction of its four 16-bit parts (exact as
 * doubles) and their negations -- where the ranks differ, the maximum of a part and minus the maximum
 * of its negation (the minimum) differ.  -> the all-reduce's code, unchanged; on XG_OK *differ says
 * whether any rank's digest differs (alike on every rank).  The refusal's words are the caller's. */
static inline int agree_digest(xg_ctx *ctx, uint64_t h, int *differ)
{
    double red[8];
    int j, rc;
    for (j = 0; j < 4; ++j) {
        red[j] = (double)((h >> (16 * j)) & 0xffff);
        red[4 + j] = -red[j];
    }
    if ((rc = xg_allreduce_max(ctx, red, 8))) return rc;
    *differ = 0;
    for (j = 0; j < 4; ++j) *differ |= red[j] != -red[4 + j];
    return XG_OK;
}

/* Whether any rank failed: one MAX reduction of (failed, code) with local_rc, this rank's result so
 * far.  With flag, a third double rides along and *flag becomes 1 on every rank when any rank's is
 * set (a choice that changes the RCCL calls posted, which no rank may make alone).  -> local_rc, or
 * the all-reduce's code, when the all-reduce itself fails; XG_OK when nobody failed; local_rc when
 * this rank did (err keeps its own words); else the highest code, err naming it and `what` the
 * ranks were doing. */
static inline int agree_peers(xg_ctx *ctx, int local_rc, int *flag, const char *what, char *err, size_t errlen)
{
    double red[3];
    int rc;
    red[0] = local_rc ? 1.0 : 0.0;
    red[1] = (double)local_rc;
    red[2] = flag && *flag ? 1.0 : 0.0;
    if ((rc = xg_allreduce_max(ctx, red, flag ? 3 : 2))) return local_rc ? local_rc : rc;
    if (flag) *flag = red[2] != 0.0;
    if (red[0] == 0.0) return XG_OK;
    if (local_rc) return local_rc;
    snprintf(err, errlen, "another GPU of the job failed (code %d) %s", (int)red[1], what);
    return (int)red[1];
}

#endif
