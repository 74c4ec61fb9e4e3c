/* late_bulk_demo.c -- plain C against include/imt.h: apply now, prove later, in the bulk form.
 *   the sequencer applies three blocks of nullifiers with imt_itree_apply_batch -- no witness, the tree stays ahead;
 *   the prover then takes the bulk witness of the SECOND block through a view at the size that block started from
 *   (imt_itree_view_bulk_witness: one low-leaf path per insertion and one shared append, nothing of the tree changed)
 *   and checks it the way the circuit would, with the stateless calls alone:
 *     per row k (descending values): imt_non_membership_batch of v[order[k]] at root_before[k]; the rewritten low leaf
 *       {low.val, v, S + order[k]} on the same path gives root_after[k] (imt_hash3_batch + imt_path_root_batch); the roots
 *       chain from the root the first block left; new_leaf[order[k]] == {v, low_leaf[k].next_val, low_leaf[k].next_idx};
 *     the append: imt_frontier_append_root(append_sib, S, new_leaf) gives root_after[n-1] before and, after, the root the
 *       sequencer reported for the second block.
 * Build:
 *   gcc -std=c11 -I include examples/late_bulk_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o late_bulk_demo
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define N 6
#define DEPTH 8

static void print_root(const unsigned char *r) {
    for (int k = 31; k >= 0; k--) printf("%02x", r[k]);
}
static void put_small(unsigned char *row, unsigned long long v) {
    memset(row, 0, 32);
    for (int k = 0; k < 8; k++) row[k] = (unsigned char)(v >> (8 * k));
}

int main(void) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL;
    imt_itree_view *view = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 64, &tree))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }

    /* ---- the sequencer: three blocks, no witness, a root per block ---- */
    static const unsigned block1[3] = {20, 50, 90}, block2[N] = {30, 70, 45, 10, 65, 25}, block3[3] = {15, 85, 60};
    unsigned char b1[3][32], vals[N][32], b3[3][32], root1[32], root2[32], root3[32];
    for (int i = 0; i < 3; i++) put_small(b1[i], block1[i]);
    for (int i = 0; i < N; i++) put_small(vals[i], block2[i]);
    for (int i = 0; i < 3; i++) put_small(b3[i], block3[i]);
    if ((rc = imt_itree_apply_batch(tree, b1, 3, root1, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    const uint64_t S = imt_itree_size(tree);                 /* where the second block starts */
    if ((rc = imt_itree_apply_batch(tree, vals, N, root2, IMT_FMT_CANONICAL)) ||
        (rc = imt_itree_apply_batch(tree, b3, 3, root3, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "%s\n", imt_last_error(ctx));
        return 1;
    }
    printf("sequencer: 3 blocks applied, %llu leaves, root ", (unsigned long long)imt_itree_size(tree));
    print_root(root3);
    printf("\n");

    /* ---- the prover, later: the bulk witness of block 2 through a view at S ---- */
    uint64_t order[N], low_index[N];
    uint8_t is_largest[N];
    unsigned char low_leaf[N][3][32], new_leaf[N][3][32], root_before[N][32], root_after[N][32], low_sib[DEPTH][N][32];
    unsigned char append_sib[DEPTH][32], root[32];
    imt_bulk_out out;
    memset(&out, 0, sizeof out);
    out.order = order;
    out.low_index = low_index;
    out.low_leaf = low_leaf;
    out.is_largest = is_largest;
    out.root_before = root_before;
    out.root_after = root_after;
    out.low_sib = low_sib;
    out.new_leaf = new_leaf;
    out.append_sib = append_sib;
    out.root = root;
    if ((rc = imt_itree_view_create(tree, S, &view)) ||
        (rc = imt_itree_view_bulk_witness(view, N, &out, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "late bulk witness: %s\n", imt_last_error(ctx));
        return 1;
    }
    for (int k = 0; k < N; k++) {
        printf("row %d: value %u (position %llu), low leaf %llu pointing at %u%s, root after ", k, block2[order[k]],
               (unsigned long long)order[k], (unsigned long long)low_index[k], (unsigned)low_leaf[k][1][0],
               is_largest[k] ? " (the largest)" : "");
        print_root(root_after[k]);
        printf("\n");
    }
    printf("append of %d leaves at slot %llu, root ", N, (unsigned long long)S);
    print_root(root);
    printf("\n");

    /* ---- the circuit's checks, with the stateless calls ---- */
    int bad = 0;
    unsigned char row_vals[N][32], rewritten[N][3][32], rewritten_hash[N][32], climbed[N][32], nm_root[N][32];
    uint8_t fail[N], seen[N];
    memset(seen, 0, sizeof seen);
    for (int k = 0; k < N; k++) {
        if (order[k] >= N || seen[order[k]]++) { bad |= 1; break; }                       /* a permutation */
        memcpy(row_vals[k], vals[order[k]], 32);
        if (k && block2[order[k]] >= block2[order[k - 1]]) bad |= 2;                      /* strictly descending */
        memcpy(rewritten[k][0], low_leaf[k][0], 32);
        memcpy(rewritten[k][1], row_vals[k], 32);
        put_small(rewritten[k][2], S + order[k]);
        if (memcmp(new_leaf[order[k]][0], row_vals[k], 32) || memcmp(new_leaf[order[k]][1], low_leaf[k][1], 64)) bad |= 4;
        if (memcmp(root_before[k], k ? root_after[k - 1] : root1, 32)) bad |= 8;          /* the roots chain from block 1's */
    }
    if (bad) { printf("late bulk witness of block 2: check mask 0x%x FAILED\n", bad); return 1; }
    if ((rc = imt_non_membership_batch(ctx, root_before, low_leaf, low_index, low_sib, DEPTH, row_vals, is_largest, N, fail,
                                       nm_root, IMT_FMT_CANONICAL | IMT_ROOT_PER_ITEM)) ||
        (rc = imt_hash3_batch(ctx, rewritten, rewritten_hash, N, IMT_FMT_CANONICAL)) ||
        (rc = imt_path_root_batch(ctx, rewritten_hash, low_index, low_sib, DEPTH, N, climbed, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "check: %s\n", imt_last_error(ctx));
        return 1;
    }
    for (int k = 0; k < N; k++)
        if (fail[k] || memcmp(climbed[k], root_after[k], 32)) bad |= 16;
    unsigned char before[32], after[32], zero[DEPTH + 1][32];
    if ((rc = imt_frontier_append_root(ctx, append_sib, S, NULL, new_leaf, N, DEPTH, before, after, IMT_FMT_CANONICAL)) ||
        (rc = imt_zero_hashes(ctx, DEPTH, zero, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "append: %s\n", imt_last_error(ctx));
        return 1;
    }
    if (memcmp(before, root_after[N - 1], 32) || memcmp(after, root, 32)) bad |= 32;
    for (int l = 0; l < DEPTH; l++)
        if (!((S >> l) & 1) && memcmp(append_sib[l], zero[l], 32)) bad |= 64;             /* right-hand siblings are Z[l] */
    if (memcmp(root, root2, 32)) bad |= 128;                                              /* the root the sequencer reported */
    unsigned char still[32];
    if ((rc = imt_itree_root(tree, still, IMT_FMT_CANONICAL))) return 1;
    if (memcmp(still, root3, 32)) bad |= 256;                                             /* and the tree is where it was */
    if (bad) {
        printf("late bulk witness of block 2: check mask 0x%x FAILED\n", bad);
        return 1;
    }
    printf("late bulk witness of block 2: %d rows and the append of %d leaves, all satisfied\n", N, N);

    imt_itree_view_free(view);
    imt_itree_free(tree);
    imt_ctx_destroy(ctx);
    return 0;
}
