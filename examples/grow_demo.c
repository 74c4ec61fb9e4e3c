/* grow_demo.c -- a follower that outgrows its tree, in plain C against include/imt.h: the nullifier tree starts with room
 * for 2^10 leaves and receives ten blocks of 300 values (imt_itree_apply_batch).  A block that does not fit comes back
 * as IMT_ERR_FULL with the tree untouched; the follower doubles the capacity of the tree it has (imt_itree_reserve: a
 * copy, no hash, same root) and applies the same block again.  Then the last seven blocks are dropped (imt_itree_rewind)
 * and the tree gives the memory back (imt_itree_reserve to the smallest capacity that holds it).  Sizes, capacities and
 * roots are printed; with an argument (64 hex digits, most significant first) the exit status says whether the final
 * root equals it.  Build:
 *   gcc -std=c11 -I include examples/grow_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o grow_demo
 * Usage: grow_demo [expected final root]
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define KEPT 3
#define PER_BLOCK 300
#define DEPTH 32

static const char *show(const unsigned char *root, char *hex) {
    for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[31 - k]);
    return hex;
}

/* item i of block j: distinct, non-zero, in no order (follow_chain.c's stream) */
static void block_values(unsigned char vals[PER_BLOCK][32], int j) {
    memset(vals, 0, (size_t)PER_BLOCK * 32);
    for (int i = 0; i < PER_BLOCK; i++) {
        const uint64_t v = 1 + 7919023757ULL * (uint64_t)(PER_BLOCK * j + i + 1) % ((1ULL << 61) - 1);
        for (int k = 0; k < 8; k++) vals[i][k] = (unsigned char)(v >> (8 * k));
    }
}

int main(int argc, char **argv) {
    imt_ctx *ctx = NULL;
    imt_itree *t = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 1 << 10, &t))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    static unsigned char vals[PER_BLOCK][32];
    unsigned char root[32], before[32], kept_root[32];
    char hex[65];
    int bad = 0;
    uint64_t kept_size = 0;
    for (int j = 0; j < BLOCKS; j++) {
        block_values(vals, j);
        rc = imt_itree_apply_batch(t, vals, PER_BLOCK, root, IMT_FMT_CANONICAL);
        if (rc == IMT_ERR_FULL) {
            /* nothing was applied; the same tree with twice the room, then the same block */
            const uint64_t cap = imt_itree_capacity(t);
            if ((rc = imt_itree_root(t, before, IMT_FMT_CANONICAL)) || (rc = imt_itree_reserve(t, 2 * cap, 0)) ||
                (rc = imt_itree_root(t, root, IMT_FMT_CANONICAL))) {
                fprintf(stderr, "block %d: %s\n", j, imt_last_error(ctx));
                return 1;
            }
            const int same = !memcmp(before, root, 32);
            printf("block %d: full at %llu of %llu leaves; capacity now %llu, root %s\n", j,
                   (unsigned long long)imt_itree_size(t), (unsigned long long)cap, (unsigned long long)imt_itree_capacity(t),
                   same ? "unchanged" : "CHANGED");
            bad |= !same;
            rc = imt_itree_apply_batch(t, vals, PER_BLOCK, root, IMT_FMT_CANONICAL);
        }
        if (rc) { fprintf(stderr, "block %d: %s\n", j, imt_last_error(ctx)); return 1; }
        if (j + 1 == KEPT) {
            memcpy(kept_root, root, 32);
            kept_size = imt_itree_size(t);
        }
    }
    printf("follower: %llu leaves of %llu, root %s\n", (unsigned long long)imt_itree_size(t),
           (unsigned long long)imt_itree_capacity(t), show(root, hex));

    /* a reorg drops the last blocks; the smallest capacity that holds what is left */
    if ((rc = imt_itree_rewind(t, kept_size, root, NULL, IMT_FMT_CANONICAL))) { fprintf(stderr, "rewind: %s\n", imt_last_error(ctx)); return 1; }
    uint64_t fit = 2;
    while (fit < kept_size) fit *= 2;
    if ((rc = imt_itree_reserve(t, fit, 0)) || (rc = imt_itree_root(t, root, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "shrink: %s\n", imt_last_error(ctx));
        return 1;
    }
    printf("after the reorg: %llu leaves of %llu, root %s\n", (unsigned long long)imt_itree_size(t),
           (unsigned long long)imt_itree_capacity(t), show(root, hex));
    const int back = !memcmp(root, kept_root, 32);
    printf("the root after block %d %s\n", KEPT - 1, back ? "is the root again" : "DIFFERS from the root now");
    bad |= !back;
    /* below the size there is nothing to shrink to */
    rc = imt_itree_reserve(t, fit / 2, 0);
    printf("a capacity below the size: %s\n", rc == IMT_ERR_RANGE && imt_itree_capacity(t) == fit ? "refused, the tree as it was"
                                                                                                  : "NOT refused as it should be");
    bad |= !(rc == IMT_ERR_RANGE && imt_itree_capacity(t) == fit);
    if (argc > 1) {
        const int off = strcmp(argv[1], hex) != 0;
        printf("final root %s\n", off ? "DIFFERS from the expected one" : "equals the expected one");
        bad |= off;
    }
    imt_itree_free(t);
    imt_ctx_destroy(ctx);
    return bad;
}
