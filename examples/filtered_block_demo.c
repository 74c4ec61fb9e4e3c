/* filtered_block_demo.c -- plain C against include/imt.h: a sequencer's block through imt_itree_mixed_filtered.
 * The block of block_demo.c, but three of its transactions are invalid: 30 is spent twice (a double spend inside the
 * block), 10 is asserted absent two transactions after the block spent it, and the last one spends 0.  45 is asserted
 * absent BEFORE the block spends it, which is legal.  imt_itree_mixed_batch would refuse the whole block and name only
 * the first offender; this call skips the three with a status each and carries out the rest, in one call.  Build:
 *   gcc -std=c11 -I include examples/filtered_block_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o filtered_block_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define N 10
#define DEPTH 8

static void print_root(const unsigned char *r) {
    for (int k = 31; k >= 0; k--) printf("%02x", r[k]);
}

int main(void) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 64, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    static const unsigned small[N] = {30, 45, 10, 30, 10, 70, 65, 45, 25, 0};
    static const uint8_t op[N] = {IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_INSERT, IMT_OP_READ,
                                  IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT};
    unsigned char vals[N][32];
    memset(vals, 0, sizeof vals);
    for (int p = 0; p < N; p++) vals[p][0] = (unsigned char)small[p];

    /* the roots of the accepted operations are all this example asks for; every other field may be NULL */
    unsigned char new_root[N][32], r_root[N][32], status[N];
    uint64_t leaf_index[N], n_ins = 0, n_rd = 0;
    imt_insert_out ins;
    imt_read_out rd;
    memset(&ins, 0, sizeof ins);
    memset(&rd, 0, sizeof rd);
    ins.new_root = new_root;
    rd.root = r_root;
    if ((rc = imt_itree_mixed_filtered(tree, vals, op, N, status, leaf_index, &ins, &rd, &n_ins, &n_rd, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "block: %s\n", imt_last_error(ctx));
        return 1;
    }
    static const char *const what[] = {"carried out", "skipped: zero", "skipped: stored before the block",
                                       "skipped: spent earlier in the block"};
    size_t r = 0, q = 0;
    for (int p = 0; p < N; p++) {
        printf("op %d: %s %u: %s, leaf %llu", p, op[p] == IMT_OP_INSERT ? "INSERT" : "READ", small[p],
               status[p] <= IMT_VAL_REPEATED ? what[status[p]] : "?", (unsigned long long)leaf_index[p]);
        if (status[p] == IMT_VAL_NEW) {
            fputs(op[p] == IMT_OP_INSERT ? ", new root " : ", against root ", stdout);
            print_root(op[p] == IMT_OP_INSERT ? new_root[r++] : r_root[q++]);
        }
        printf("\n");
    }
    unsigned char root[32];
    if ((rc = imt_itree_root(tree, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "root: %s\n", imt_last_error(ctx)); return 1; }
    printf("block of %d operations: %llu inserted, %llu read, %llu skipped; final root ", N, (unsigned long long)n_ins,
           (unsigned long long)n_rd, (unsigned long long)(N - n_ins - n_rd));
    print_root(root);
    printf("\n");
    const int ok = r == n_ins && q == n_rd && n_ins == 4 && n_rd == 3 && imt_itree_size(tree) == 1 + n_ins &&
                   (n_ins == 0 || !memcmp(root, new_root[n_ins - 1], 32));
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return !ok;
}
