/* nullifier_demo.c -- plain C against include/imt.h: nullifiers derived on the GPU that inserts them.
 * Each transaction spends a note; its nullifier is the Poseidon hash of four fields {commitment, key, position, domain},
 * the hash the circuit computes with the same hasher it hands to the tree chip.  imt_hash_n_batch derives all of them in
 * one call and imt_itree_insert_filtered takes the results as they are: the fifth transaction spends the note of the
 * second again, so its nullifier comes out equal and is skipped as a double spend.  Build:
 *   gcc -std=c11 -I include examples/nullifier_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o nullifier_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define N 6
#define FIELDS 4
#define DEPTH 8

static void print_fe(const unsigned char *r) {
    for (int k = 31; k >= 0; k--) printf("%02x", r[k]);
}

int main(void) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 64, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    /* {commitment, key, position, domain} per transaction, small integers for the sake of the printout */
    static const unsigned note[N][FIELDS] = {{101, 7, 0, 1}, {102, 7, 1, 1}, {103, 9, 2, 1},
                                             {104, 9, 3, 1}, {102, 7, 1, 1}, {105, 11, 4, 1}};
    unsigned char pre[N][FIELDS][32], nullifier[N][32];
    memset(pre, 0, sizeof pre);
    for (int i = 0; i < N; i++)
        for (int j = 0; j < FIELDS; j++) pre[i][j][0] = (unsigned char)note[i][j];
    if ((rc = imt_hash_n_batch(ctx, pre, FIELDS, nullifier, N, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "imt_hash_n_batch: %s\n", imt_last_error(ctx));
        return 1;
    }

    unsigned char status[N], root[32];
    uint64_t leaf_index[N], n_inserted = 0;
    if ((rc = imt_itree_insert_filtered(tree, nullifier, N, status, leaf_index, &n_inserted, NULL, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "imt_itree_insert_filtered: %s\n", imt_last_error(ctx));
        return 1;
    }
    for (int i = 0; i < N; i++) {
        printf("tx %d: nullifier ", i);
        print_fe(nullifier[i]);
        printf(status[i] == IMT_VAL_NEW ? ": inserted at leaf %llu\n" : ": double spend, first seen at leaf %llu\n",
               (unsigned long long)leaf_index[i]);
    }
    if ((rc = imt_itree_root(tree, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "root: %s\n", imt_last_error(ctx)); return 1; }
    printf("%d transactions: %llu nullifiers inserted, %llu skipped; root ", N, (unsigned long long)n_inserted,
           (unsigned long long)(N - n_inserted));
    print_fe(root);
    printf("\n");
    const int ok = n_inserted == N - 1 && status[4] == IMT_VAL_REPEATED && leaf_index[4] == leaf_index[1] &&
                   !memcmp(nullifier[4], nullifier[1], 32) && imt_itree_size(tree) == 1 + n_inserted;
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return !ok;
}
