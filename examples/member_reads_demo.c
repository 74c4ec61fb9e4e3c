/* member_reads_demo.c -- plain C against include/imt.h: emit a nullifier, then prove that it exists, in ONE block.
 * Transaction 1 of the block inserts 45 (insert_leaf); transaction 3 asserts that 45 IS in the tree as of its place
 * (IMT_OP_MEMBER under IMT_MEMBER_OPS), and so does transaction 4 for 30, which was stored before the block.  The block is
 * one call of imt_itree_mixed_batch; every MEMBER row is then checked the way a consumer checks it -- low_leaf.val is the
 * value, and hash3(low_leaf) at low_index hashes up to the root the row names.  A second block that asserts the presence
 * of a value its own LATER transaction inserts is refused, and the call says where.  Build:
 *   gcc -std=c11 -I include examples/member_reads_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o member_reads_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define N 6
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

    /* before the block: 30 and 60 are in the tree */
    unsigned char stored[2][32], root[32];
    memset(stored, 0, sizeof stored);
    stored[0][0] = 30;
    stored[1][0] = 60;
    if ((rc = imt_itree_apply_batch(tree, stored, 2, root, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    /* the block: 45 is absent at operation 0, emitted at operation 1 and proved present at operation 3 */
    static const unsigned small[N] = {45, 45, 50, 45, 30, 60};
    static const uint8_t op[N] = {IMT_OP_READ, IMT_OP_INSERT, IMT_OP_INSERT, IMT_OP_MEMBER, IMT_OP_MEMBER, IMT_OP_MEMBER};
    unsigned char vals[N][32];
    memset(vals, 0, sizeof vals);
    for (int p = 0; p < N; p++) vals[p][0] = (unsigned char)small[p];

    /* rows of the operations that are no INSERT: READs and MEMBERs share one numbering in block order */
    uint64_t r_low_index[N];
    unsigned char r_is_largest[N], r_low_leaf[N][3][32], r_root[N][32], r_low_sib[DEPTH][N][32];
    imt_read_out rd = {r_low_index, r_low_leaf, r_is_largest, r_root, r_low_sib};
    uint64_t n_ins = 0, bad_op = 0;
    if ((rc = imt_itree_mixed_batch(tree, vals, op, N, NULL, &rd, &n_ins, &bad_op, IMT_FMT_CANONICAL | IMT_MEMBER_OPS))) {
        fprintf(stderr, "block: %s\n", imt_last_error(ctx));
        return 1;
    }
    const size_t n_rd = N - (size_t)n_ins;

    /* the consumer's check of every row: the leaf hash, then the path to the root the row names.  The sibling array keeps
     * the level stride N, so the rows are gathered item-major first */
    unsigned char leaf_hash[N][32], ok[N], ri[N][DEPTH][32];
    for (int l = 0; l < DEPTH; l++)
        for (int i = 0; i < N; i++) memcpy(ri[i][l], r_low_sib[l][i], 32);
    if ((rc = imt_hash3_batch(ctx, r_low_leaf, leaf_hash, n_rd, IMT_FMT_CANONICAL)) ||
        (rc = imt_verify_proof_batch(ctx, leaf_hash, r_low_index, r_root, ri, DEPTH, n_rd, ok,
                                     IMT_FMT_CANONICAL | IMT_SIB_ITEM_MAJOR | IMT_ROOT_PER_ITEM))) {
        fprintf(stderr, "check: %s\n", imt_last_error(ctx));
        return 1;
    }
    size_t q = 0;
    int bad_rows = 0;
    for (int p = 0; p < N; p++) {
        if (op[p] == IMT_OP_INSERT) continue;
        const int member = op[p] == IMT_OP_MEMBER;
        const int holds = memcmp(r_low_leaf[q][0], vals[p], 32) == 0;       /* low_leaf.val == v: a MEMBER's row, never a READ's */
        printf("op %d: %2u is %s: leaf %llu {%u -> %u}%s, against root ", p, small[p], member ? "present" : "absent ",
               (unsigned long long)r_low_index[q], (unsigned)r_low_leaf[q][0][0], (unsigned)r_low_leaf[q][1][0],
               r_is_largest[q] ? " (the largest)" : "");
        print_root(r_root[q]);
        printf("\n");
        if (!ok[q] || holds != member) bad_rows++;
        q++;
    }
    printf("block of %d: %llu inserted, %zu rows, %d bad\n", N, (unsigned long long)n_ins, n_rd, bad_rows);
    if (bad_rows || n_ins != 2 || q != n_rd) return 1;

    /* a later INSERT does not help: 70 is asserted present at operation 0 and emitted at operation 1 */
    unsigned char late[2][32];
    static const uint8_t late_op[2] = {IMT_OP_MEMBER, IMT_OP_INSERT};
    memset(late, 0, sizeof late);
    late[0][0] = late[1][0] = 70;
    rc = imt_itree_mixed_batch(tree, late, late_op, 2, NULL, NULL, NULL, &bad_op, IMT_FMT_CANONICAL | IMT_MEMBER_OPS);
    if (rc != IMT_ERR_VALUE || bad_op != 0) { fprintf(stderr, "the second block was not refused at operation 0 (%d)\n", rc); return 1; }
    printf("second block refused: %s\n", imt_last_error(ctx));

    /* and without the flag the third kind does not exist */
    rc = imt_itree_mixed_batch(tree, vals, op, N, NULL, NULL, NULL, NULL, IMT_FMT_CANONICAL);
    if (rc != IMT_ERR_ARG) { fprintf(stderr, "op byte 2 was accepted without IMT_MEMBER_OPS (%d)\n", rc); return 1; }
    if ((rc = imt_itree_root(tree, root, IMT_FMT_CANONICAL))) return 1;
    printf("root ");
    print_root(root);
    printf("\nmember reads demo ok\n");
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return 0;
}
