/* block_demo.c -- plain C against include/imt.h: one block of interleaved transactions through imt_itree_mixed_batch.
 * Some transactions insert a nullifier (insert_leaf), others only assert that a value is absent
 * (verify_non_inclusion) against the tree as it stands at that point of the block; the block is one call, and every
 * row is then re-checked on the GPU by the two relation checkers -- the INSERT rows as insert_leaf witnesses, the READ
 * rows as non-inclusion witnesses against the root each of them names.  A second block that asserts the absence of a
 * value the block itself inserted earlier is refused, and the call says where.  Build:
 *   gcc -std=c11 -I include examples/block_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o block_demo
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

    /* the block: 45 is absent at operation 1 and inserted at operation 7; 65 lies above everything at operation 4 and
     * below 70 at operation 6 */
    static const unsigned small[N] = {30, 45, 10, 60, 65, 70, 65, 45, 25, 5};
    static const uint8_t op[N] = {IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_INSERT, IMT_OP_READ,
                                  IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT, IMT_OP_READ,   IMT_OP_INSERT};
    unsigned char vals[N][32];
    memset(vals, 0, sizeof vals);
    for (int p = 0; p < N; p++) vals[p][0] = (unsigned char)small[p];

    /* rows of the INSERTs and of the READs; sibling arrays are dimensioned for the N operations */
    uint64_t low_index[N], new_index[N], r_low_index[N];
    unsigned char is_largest[N], low_leaf[N][3][32], new_leaf[N][3][32], old_root[N][32], interim_root[N][32], new_root[N][32];
    unsigned char low_sib[DEPTH][N][32], new_sib[DEPTH][N][32];
    unsigned char r_is_largest[N], r_low_leaf[N][3][32], r_root[N][32], r_low_sib[DEPTH][N][32], r_vals[N][32];
    imt_insert_out ins = {low_index, low_leaf, is_largest, old_root, interim_root, new_root, new_leaf, low_sib, new_sib};
    imt_read_out rd = {r_low_index, r_low_leaf, r_is_largest, r_root, r_low_sib};
    uint64_t n_ins = 0, bad_op = 0;
    if ((rc = imt_itree_mixed_batch(tree, vals, op, N, &ins, &rd, &n_ins, &bad_op, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "block: %s\n", imt_last_error(ctx));
        return 1;
    }
    const size_t n_rd = N - (size_t)n_ins;
    size_t r = 0, q = 0;
    for (int p = 0; p < N; p++) {
        if (op[p] == IMT_OP_INSERT) {
            new_index[r] = 1 + r;
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

    /* a block that reads 80 after inserting it is no block: refused, nothing changed, and the call names the position */
    unsigned char root_before[32], root_after[32], blk[3][32];
    static const uint8_t op2[3] = {IMT_OP_READ, IMT_OP_INSERT, IMT_OP_READ};
    memset(blk, 0, sizeof blk);
    blk[0][0] = blk[1][0] = blk[2][0] = 80;
    rc = imt_itree_root(tree, root_before, IMT_FMT_CANONICAL);
    const int rc2 = imt_itree_mixed_batch(tree, blk, op2, 3, NULL, NULL, NULL, &bad_op, IMT_FMT_CANONICAL);
    if (!rc) rc = imt_itree_root(tree, root_after, IMT_FMT_CANONICAL);
    if (rc) { fprintf(stderr, "root: %s\n", imt_last_error(ctx)); return 1; }
    const int refused = rc2 == IMT_ERR_VALUE && bad_op == 2 && !memcmp(root_before, root_after, 32);
    printf("read-after-insert block: %s at operation %llu, root %s\n", rc2 == IMT_ERR_VALUE ? "refused" : "ACCEPTED",
           (unsigned long long)bad_op, memcmp(root_before, root_after, 32) ? "CHANGED" : "unchanged");
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return bad != 0 || !refused;
}
