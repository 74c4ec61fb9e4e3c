/* apply_block_demo.c -- plain C against include/imt.h: a sequencer applies a block now and proves it later.
 * The block of filtered_block_demo.c: 30 is spent twice (a double spend inside the block), 10 is asserted absent two
 * transactions after the block spent it, and the last one spends 0; 45 is asserted absent BEFORE the block spends it,
 * which is legal.  imt_itree_apply_mixed_filtered skips the three with a status each and applies the rest without a
 * single witness: every touched node hashed once, no hash for a READ.  Later -- here: right away -- a view of the tree at
 * the size before the block replays the operations that were carried out through imt_itree_view_mixed_witness and gets
 * the roots the prover needs.  Build:
 *   gcc -std=c11 -I include examples/apply_block_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o apply_block_demo
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
    imt_itree_view *view = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 64, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    static const unsigned small[N] = {30, 45, 10, 30, 10, 70, 65, 45, 25, 0};
    static const uint8_t op[N] = {IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_INSERT, IMT_OP_READ,
                                  IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT};
    unsigned char vals[N][32];
    memset(vals, 0, sizeof vals);
    for (int p = 0; p < N; p++) vals[p][0] = (unsigned char)small[p];

    /* ---- now: the block into the tree, statuses and the root after it, nothing else ---- */
    const uint64_t size_before = imt_itree_size(tree);
    unsigned char status[N], applied_root[32];
    uint64_t leaf_index[N], n_ins = 0, n_rd = 0;
    if ((rc = imt_itree_apply_mixed_filtered(tree, vals, op, N, status, leaf_index, &n_ins, &n_rd, applied_root,
                                             IMT_FMT_CANONICAL))) {
        fprintf(stderr, "block: %s\n", imt_last_error(ctx));
        return 1;
    }
    static const char *const what[] = {"carried out", "skipped: zero", "skipped: stored before the block",
                                       "skipped: spent earlier in the block"};
    for (int p = 0; p < N; p++)
        printf("op %d: %s %u: %s, leaf %llu\n", p, op[p] == IMT_OP_INSERT ? "INSERT" : "READ", small[p],
               status[p] <= IMT_VAL_REPEATED ? what[status[p]] : "?", (unsigned long long)leaf_index[p]);
    printf("block of %d operations: %llu inserted, %llu read, %llu skipped; applied root ", N, (unsigned long long)n_ins,
           (unsigned long long)n_rd, (unsigned long long)(N - n_ins - n_rd));
    print_root(applied_root);
    printf("\n");

    /* ---- later: the witnesses of the operations that were carried out, from a view at the size before the block ---- */
    unsigned char acc_vals[N][32], new_root[N][32], r_root[N][32];
    uint8_t acc_op[N];
    int acc_pos[N];
    size_t n_acc = 0;
    for (int p = 0; p < N; p++)
        if (status[p] == IMT_VAL_NEW) {
            memcpy(acc_vals[n_acc], vals[p], 32);
            acc_op[n_acc] = op[p];
            acc_pos[n_acc++] = p;
        }
    imt_insert_out ins;
    imt_read_out rd;
    memset(&ins, 0, sizeof ins);
    memset(&rd, 0, sizeof rd);
    ins.new_root = new_root;
    rd.root = r_root;
    uint64_t replayed = 0;
    if ((rc = imt_itree_view_create(tree, size_before, &view)) ||
        (rc = imt_itree_view_mixed_witness(view, acc_vals, acc_op, n_acc, &ins, &rd, &replayed, NULL, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "replay: %s\n", imt_last_error(ctx));
        return 1;
    }
    size_t r = 0, q = 0;
    for (size_t k = 0; k < n_acc; k++) {
        const int insert = acc_op[k] == IMT_OP_INSERT;
        printf("proved op %d: %s", acc_pos[k], insert ? "new root " : "against root ");
        print_root(insert ? new_root[r++] : r_root[q++]);
        printf("\n");
    }
    unsigned char root[32];
    if ((rc = imt_itree_root(tree, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "root: %s\n", imt_last_error(ctx)); return 1; }
    printf("final root ");
    print_root(root);
    printf("\n");
    const int ok = n_ins == 4 && n_rd == 3 && n_acc == n_ins + n_rd && replayed == n_ins && r == n_ins && q == n_rd &&
                   imt_itree_size(tree) == size_before + n_ins && !memcmp(root, applied_root, 32) &&
                   !memcmp(root, new_root[n_ins - 1], 32);
    imt_itree_view_free(view);
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return !ok;
}
