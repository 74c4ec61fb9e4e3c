/* reorg_demo.c -- a reorg in plain C against include/imt.h: a node that keeps the nullifier tree current applies ten
 * blocks of 64 values (imt_itree_apply_batch), learns that the last three blocks were dropped, goes back to the tree it
 * had after block 6 (imt_itree_rewind: nothing is needed but the size, no snapshot was taken) and applies the three
 * blocks of the branch that won.  The root after every step is printed.  With an argument (64 hex digits, most
 * significant first) the last root is compared with it and the exit status says whether they are equal.  Build:
 *   gcc -std=c11 -I include examples/reorg_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o reorg_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define DROPPED 3
#define PER_BLOCK 64
#define DEPTH 32

static char hex[65];
static const char *show(const unsigned char *root) {
    for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[31 - k]);
    return hex;
}

/* item i of block j of branch b: distinct, non-zero, in no order (branch 0 is follow_chain.c's stream) */
static void block_values(unsigned char vals[PER_BLOCK][32], int branch, int j) {
    memset(vals, 0, (size_t)PER_BLOCK * 32);
    for (int i = 0; i < PER_BLOCK; i++) {
        const uint64_t x = (uint64_t)(PER_BLOCK * j + i + 1) + (branch ? 1000000u : 0u);
        const uint64_t v = 1 + 7919023757ULL * x % ((1ULL << 61) - 1);
        for (int k = 0; k < 8; k++) vals[i][k] = (unsigned char)(v >> (8 * k));
    }
}

int main(int argc, char **argv) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 1024, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    unsigned char vals[PER_BLOCK][32], root[32];
    uint64_t hashes[DEPTH + 1], total = 0;
    for (int j = 0; j < BLOCKS; j++) {
        block_values(vals, 0, j);
        if ((rc = imt_itree_apply_batch(tree, vals, PER_BLOCK, root, IMT_FMT_CANONICAL))) {
            fprintf(stderr, "block %d: %s\n", j, imt_last_error(ctx));
            return 1;
        }
        printf("block %d: root %s\n", j, show(root));
    }
    /* the last DROPPED blocks are gone: the tree of 1 + 7 * 64 leaves again */
    const uint64_t keep = 1 + (uint64_t)(BLOCKS - DROPPED) * PER_BLOCK;
    if ((rc = imt_itree_rewind(tree, keep, root, hashes, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "rewind: %s\n", imt_last_error(ctx));
        return 1;
    }
    for (int l = 0; l <= DEPTH; l++) total += hashes[l];
    printf("rewind to %llu leaves: root %s (%llu hashes for %d insertions undone)\n", (unsigned long long)keep, show(root),
           (unsigned long long)total, DROPPED * PER_BLOCK);
    for (int j = BLOCKS - DROPPED; j < BLOCKS; j++) {
        block_values(vals, 1, j);
        if ((rc = imt_itree_apply_batch(tree, vals, PER_BLOCK, root, IMT_FMT_CANONICAL))) {
            fprintf(stderr, "fork block %d: %s\n", j, imt_last_error(ctx));
            return 1;
        }
        printf("fork block %d: root %s\n", j, show(root));
    }
    int bad = 0;
    if (argc > 1) {
        bad = strcmp(argv[1], show(root)) != 0;
        printf("final root %s\n", bad ? "DIFFERS from the expected one" : "equals the expected one");
    }
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return bad;
}
