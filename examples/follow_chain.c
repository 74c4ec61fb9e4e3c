/* follow_chain.c -- "follow the chain" in plain C against include/imt.h: a node that keeps the nullifier tree current
 * and proves nothing applies every block's values with imt_itree_apply_batch (one hash per touched node, no witnesses)
 * and compares each block's root with the one the chain announced.  Ten blocks of 64 values into a depth-32 tree; the
 * root after every block is printed.  With an argument (64 hex digits, most significant first) the last root is
 * compared with it and the exit status says whether they are equal.  Build:
 *   gcc -std=c11 -I include examples/follow_chain.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o follow_chain
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define PER_BLOCK 64
#define DEPTH 32

int main(int argc, char **argv) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 1024, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    unsigned char vals[PER_BLOCK][32], root[32];
    char hex[65] = {0};
    uint64_t total = 0, hashes[DEPTH + 1];
    for (int j = 0; j < BLOCKS; j++) {
        memset(vals, 0, sizeof vals);
        for (int i = 0; i < PER_BLOCK; i++) {         /* a block's nullifiers: distinct, non-zero, in no order */
            const uint64_t v = 1 + 7919023757ULL * (uint64_t)(PER_BLOCK * j + i + 1) % ((1ULL << 61) - 1);
            for (int k = 0; k < 8; k++) vals[i][k] = (unsigned char)(v >> (8 * k));
        }
        if ((rc = imt_itree_apply_batch(tree, vals, PER_BLOCK, root, IMT_FMT_CANONICAL)) ||
            (rc = imt_itree_apply_stats(tree, hashes))) {
            fprintf(stderr, "block %d: %s\n", j, imt_last_error(ctx));
            return 1;
        }
        for (int l = 0; l <= DEPTH; l++) total += hashes[l];
        for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[31 - k]);
        printf("block %d: root %s\n", j, hex);
    }
    printf("%d values applied with %llu hashes (the witness sweep: %d)\n", BLOCKS * PER_BLOCK, (unsigned long long)total,
           BLOCKS * PER_BLOCK * (2 + 2 * DEPTH));
    int bad = 0;
    if (argc > 1) {
        bad = strcmp(argv[1], hex) != 0;
        printf("final root %s\n", bad ? "DIFFERS from the expected one" : "equals the expected one");
    }
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return bad;
}
