/* late_block_demo.c -- plain C against include/imt.h: apply a mixed block now, prove it later.
 * A sequencer has a block of interleaved transactions -- some insert a nullifier (insert_leaf), others only assert that
 * a value is absent (verify_non_inclusion) at that point of the block.  It applies the block's insertions witness-free
 * (imt_itree_apply_batch) and goes straight on to the next block.  A prover then makes a view of the tree at the first
 * block's start and asks for the block's witnesses with imt_itree_view_mixed_witness: every INSERT's and every READ's row
 * against the tree as it stood at that point of the block, while the tree stays two blocks ahead.  Every row is
 * re-checked on the GPU by the two relation checkers.  The same block with one transaction altered is not the block the
 * tree applied: refused, and the call says where.  Build:
 *   gcc -std=c11 -I include examples/late_block_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o late_block_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define N 10
#define DEPTH 8

static void print_root(const unsigned char *r) {
    for (int k = 31; k >= 0; k--) printf("%02x", r[k]);
}

static void small_values(unsigned char (*out)[32], const unsigned *small, int n) {
    memset(out, 0, (size_t)n * 32);
    for (int i = 0; i < n; i++) out[i][0] = (unsigned char)small[i];
}

int main(void) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    imt_itree_view *view = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 64, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    /* ---- the sequencer ---- */
    static const unsigned before[2] = {20, 40};
    static const unsigned small[N] = {30, 45, 10, 60, 65, 70, 65, 45, 25, 5};
    static const uint8_t op[N] = {IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_INSERT, IMT_OP_READ,
                                  IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT};
    static const unsigned next_block[4] = {15, 35, 55, 65};
    unsigned char v0[2][32], vals[N][32], applied[N][32], v2[4][32], root[32], head[32];
    small_values(v0, before, 2);
    small_values(vals, small, N);
    small_values(v2, next_block, 4);
    size_t k = 0;
    for (int p = 0; p < N; p++)
        if (op[p] == IMT_OP_INSERT) memcpy(applied[k++], vals[p], 32);
    if ((rc = imt_itree_apply_batch(tree, v0, 2, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    const uint64_t start = imt_itree_size(tree);
    printf("root before the block ");
    print_root(root);
    if ((rc = imt_itree_apply_batch(tree, applied, k, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    printf("\nroot after the block ");
    print_root(root);
    if ((rc = imt_itree_apply_batch(tree, v2, 4, head, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    printf("\nroot after the next block ");
    print_root(head);
    printf("\n");

    /* ---- the prover, later: a view at the block's start, the block as it was ---- */
    if ((rc = imt_itree_view_create(tree, start, &view)) || (rc = imt_itree_view_root(view, root, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "view: %s\n", imt_last_error(ctx));
        return 1;
    }
    printf("the view's root ");
    print_root(root);
    printf("\n");
    uint64_t low_index[N], new_index[N], r_low_index[N];
    unsigned char is_largest[N], low_leaf[N][3][32], new_leaf[N][3][32], old_root[N][32], interim_root[N][32], new_root[N][32];
    unsigned char low_sib[DEPTH][N][32], new_sib[DEPTH][N][32];
    unsigned char r_is_largest[N], r_low_leaf[N][3][32], r_root[N][32], r_low_sib[DEPTH][N][32], r_vals[N][32];
    imt_insert_out ins = {low_index, low_leaf, is_largest, old_root, interim_root, new_root, new_leaf, low_sib, new_sib};
    imt_read_out rd = {r_low_index, r_low_leaf, r_is_largest, r_root, r_low_sib};
    uint64_t n_ins = 0, bad_op = 0;
    if ((rc = imt_itree_view_mixed_witness(view, vals, op, N, &ins, &rd, &n_ins, &bad_op, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "replay: %s\n", imt_last_error(ctx));
        return 1;
    }
    const size_t n_rd = N - (size_t)n_ins;
    size_t r = 0, q = 0;
    for (int p = 0; p < N; p++) {
        if (op[p] == IMT_OP_INSERT) {
            new_index[r] = start + r;
            printf("op %d: insert %2u at leaf %llu, low leaf %llu, new root ", p, small[p], (unsigned long long)new_index[r],
                   (unsigned long long)low_index[r]);
            print_root(new_root[r++]);
        } else {
            memcpy(r_vals[q], vals[p], 32);
            printf("op %d: %2u is absent: low leaf %llu%s, against root ", p, small[p], (unsigned long long)r_low_index[q],
                   r_is_largest[q] ? " (the largest)" : "");
            print_root(r_root[q++]);
        }
        printf("\n");
    }

    /* every row through the relation checkers; the sibling arrays keep the level stride N, so the rows of each kind are
     * gathered item-major first */
    unsigned char li[N][DEPTH][32], ni[N][DEPTH][32], ri[N][DEPTH][32], fail[N];
    for (int l = 0; l < DEPTH; l++)
        for (int i = 0; i < N; i++) {
            memcpy(li[i][l], low_sib[l][i], 32);
            memcpy(ni[i][l], new_sib[l][i], 32);
            memcpy(ri[i][l], r_low_sib[l][i], 32);
        }
    int bad = 0;
    rc = imt_insert_witness_batch(ctx, old_root, low_leaf, low_index, li, new_root, new_leaf, new_index, NULL, ni, is_largest,
                                  DEPTH, (size_t)n_ins, fail, NULL, IMT_FMT_CANONICAL | IMT_SIB_ITEM_MAJOR);
    if (rc) { fprintf(stderr, "insert witnesses: %s\n", imt_last_error(ctx)); return 1; }
    for (size_t i = 0; i < (size_t)n_ins; i++) bad |= fail[i];
    rc = imt_non_membership_batch(ctx, r_root, r_low_leaf, r_low_index, ri, DEPTH, r_vals, r_is_largest, n_rd, fail, NULL,
                                  IMT_FMT_CANONICAL | IMT_SIB_ITEM_MAJOR | IMT_ROOT_PER_ITEM);
    if (rc) { fprintf(stderr, "read witnesses: %s\n", imt_last_error(ctx)); return 1; }
    for (size_t i = 0; i < n_rd; i++) bad |= fail[i];
    printf("block of %d operations: %llu insert_leaf and %zu verify_non_inclusion witnesses, %s\n", N,
           (unsigned long long)n_ins, n_rd, bad ? "VIOLATED" : "all satisfied");
    if ((rc = imt_itree_root(tree, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "root: %s\n", imt_last_error(ctx)); return 1; }
    const int moved = memcmp(root, head, 32) != 0;
    printf("the tree is %s: root ", moved ? "NOT where it was" : "where it was");
    print_root(root);
    printf("\n");

    /* the block with its fourth transaction altered (61 for 60) is not the block the tree applied */
    vals[3][0] = 61;
    const int rc2 = imt_itree_view_mixed_witness(view, vals, op, N, NULL, NULL, NULL, &bad_op, IMT_FMT_CANONICAL);
    const int refused = rc2 == IMT_ERR_VALUE && bad_op == 3;
    printf("altered block: %s at operation %llu\n", rc2 == IMT_ERR_VALUE ? "refused" : "ACCEPTED", (unsigned long long)bad_op);
    imt_itree_view_free(view);
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return bad != 0 || moved || !refused;
}
