/* finalized_reads_demo.c -- reads against a root that lags the head, in plain C against include/imt.h: a sequencer's
 * tree advances block by block (imt_itree_apply_batch, ten blocks of 64 values) while a non-membership service answers
 * against the FINALIZED root, three blocks back.  The service holds a view of the tree at the finalized size
 * (imt_itree_view_create): no second tree, no rewind, the head is never taken away.  After every block the view moves one
 * block on, and the values of the block just applied -- not yet finalized, so absent as of the view -- get their
 * non-membership witnesses from it, which imt_non_membership_batch verifies against the view's root.  Both roots are
 * printed after every block, and at the end the root as of the last finalized size.  With an argument (64 hex digits, most
 * significant first) that root is compared with it and the exit status says whether they are equal.  Build:
 *   gcc -std=c11 -I include examples/finalized_reads_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip \
 *       -o finalized_reads_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define LAG 3
#define PER_BLOCK 64
#define DEPTH 32

static char hex[65];
static const char *show(const unsigned char *root) {
    for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[31 - k]);
    return hex;
}

/* item i of block j: distinct, non-zero, in no order (follow_chain.c's stream) */
static void block_values(unsigned char vals[PER_BLOCK][32], int j) {
    memset(vals, 0, (size_t)PER_BLOCK * 32);
    for (int i = 0; i < PER_BLOCK; i++) {
        const uint64_t x = (uint64_t)(PER_BLOCK * j + i + 1);
        const uint64_t v = 1 + 7919023757ULL * x % ((1ULL << 61) - 1);
        for (int k = 0; k < 8; k++) vals[i][k] = (unsigned char)(v >> (8 * k));
    }
}

static unsigned char low_sib[DEPTH][PER_BLOCK][32];

int main(int argc, char **argv) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    imt_itree_view *fin = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 1024, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    unsigned char vals[PER_BLOCK][32], head[32], root[32], low_leaf[PER_BLOCK][3][32];
    uint64_t low_index[PER_BLOCK], size_after[BLOCKS], fin_size = 0;
    uint8_t largest[PER_BLOCK], fail[PER_BLOCK];
    for (int j = 0; j < BLOCKS; j++) {
        block_values(vals, j);
        if ((rc = imt_itree_apply_batch(tree, vals, PER_BLOCK, head, IMT_FMT_CANONICAL))) {
            fprintf(stderr, "block %d: %s\n", j, imt_last_error(ctx));
            return 1;
        }
        size_after[j] = imt_itree_size(tree);
        printf("head block %d: root %s\n", j, show(head));
        if (j < LAG) continue;
        /* block j - LAG is final now: the view moves there (the tree's size after that block is all it takes) */
        imt_itree_view_free(fin);
        fin_size = size_after[j - LAG];
        if ((rc = imt_itree_view_create(tree, fin_size, &fin)) || (rc = imt_itree_view_root(fin, root, IMT_FMT_CANONICAL))) {
            fprintf(stderr, "view at %llu: %s\n", (unsigned long long)fin_size, imt_last_error(ctx));
            return 1;
        }
        printf("  finalized block %d (%llu leaves): root %s\n", j - LAG, (unsigned long long)fin_size, show(root));
        /* "was any value of block j spent as of the finalized root?"  None was: each has a witness against that root */
        if ((rc = imt_itree_view_non_membership_witness(fin, vals, PER_BLOCK, low_index, low_leaf, largest, low_sib,
                                                        IMT_FMT_CANONICAL)) ||
            (rc = imt_non_membership_batch(ctx, root, low_leaf, low_index, low_sib, DEPTH, vals, largest, PER_BLOCK, fail, NULL,
                                           IMT_FMT_CANONICAL))) {
            fprintf(stderr, "witnesses at %llu: %s\n", (unsigned long long)fin_size, imt_last_error(ctx));
            return 1;
        }
        int failed = 0;
        for (int i = 0; i < PER_BLOCK; i++) failed += fail[i] != 0;
        printf("  %d non-membership witnesses against it, %d failed\n", PER_BLOCK, failed);
        if (failed) return 1;
    }
    /* the head has not moved for the service: the tree still answers with its own root */
    if ((rc = imt_itree_root(tree, root, IMT_FMT_CANONICAL)) || memcmp(root, head, 32)) {
        fprintf(stderr, "the head's root changed\n");
        return 1;
    }
    if ((rc = imt_itree_view_root(fin, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    printf("as of %llu leaves: root %s\n", (unsigned long long)fin_size, show(root));
    int bad = 0;
    if (argc > 1) {
        bad = strcmp(argv[1], show(root)) != 0;
        printf("that root %s\n", bad ? "DIFFERS from the expected one" : "equals the expected one");
    }
    imt_itree_view_free(fin);
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return bad;
}
