/* cold_start_demo.c -- a cold start in plain C against include/imt.h: a follower grows the nullifier tree by ten blocks
 * of 64 values (imt_itree_apply_batch), writes the tree's value log to a file (imt_itree_get_values: 32 bytes per leaf,
 * where the preimage snapshot of imt_itree_get_leaves has 96), and a second tree starts from that file alone
 * (imt_itree_load_values).  Both roots and the two snapshot sizes are printed; the exit status says whether the roots are
 * equal and, with an argument (64 hex digits, most significant first), whether they equal it.  A log with one value
 * repeated is then refused with the position named and the second tree as it was.  Build:
 *   gcc -std=c11 -I include examples/cold_start_demo.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o cold_start_demo
 * Usage: cold_start_demo [expected root [log file]]      (the log goes to cold_start_demo.values by default)
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define PER_BLOCK 64
#define DEPTH 32

static const char *show(const unsigned char *root, char *hex) {
    for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[31 - k]);
    return hex;
}

/* item i of block j: distinct, non-zero, in no order (follow_chain.c's stream) */
static void block_values(unsigned char vals[PER_BLOCK][32], int j) {
    memset(vals, 0, (size_t)PER_BLOCK * 32);
    for (int i = 0; i < PER_BLOCK; i++) {
        const uint64_t v = 1 + 7919023757ULL * (uint64_t)(PER_BLOCK * j + i + 1) % ((1ULL << 61) - 1);
        for (int k = 0; k < 8; k++) vals[i][k] = (unsigned char)(v >> (8 * k));
    }
}

int main(int argc, char **argv) {
    const char *path = argc > 2 ? argv[2] : "cold_start_demo.values";
    imt_ctx *ctx = NULL;
    imt_itree *follower = NULL, *cold = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if ((rc = imt_itree_new(ctx, DEPTH, 1024, &follower)) || (rc = imt_itree_new(ctx, DEPTH, 1024, &cold))) {
        fprintf(stderr, "%s\n", imt_last_error(ctx));
        return 1;
    }
    unsigned char vals[PER_BLOCK][32], root_a[32], root_b[32];
    char hex_a[65], hex_b[65];
    for (int j = 0; j < BLOCKS; j++) {
        block_values(vals, j);
        if ((rc = imt_itree_apply_batch(follower, vals, PER_BLOCK, root_a, IMT_FMT_CANONICAL))) {
            fprintf(stderr, "block %d: %s\n", j, imt_last_error(ctx));
            return 1;
        }
    }
    /* the value log: leaves 1 .. size - 1 (leaf 0 is the sentinel, which every tree has) */
    const uint64_t size = imt_itree_size(follower);
    const size_t n = (size_t)(size - 1);
    unsigned char *log = malloc(n * 32 + 32);
    if (!log) return 1;
    if ((rc = imt_itree_get_values(follower, 1, n, log, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "get_values: %s\n", imt_last_error(ctx));
        return 1;
    }
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(log, 32, n, f) != n || fclose(f)) { fprintf(stderr, "cannot write %s\n", path); return 1; }
    printf("follower: %llu leaves, root %s\n", (unsigned long long)size, show(root_a, hex_a));
    printf("value log %s: %llu bytes (a preimage snapshot of the same tree: %llu bytes)\n", path,
           (unsigned long long)(n * 32), (unsigned long long)(size * 96));

    /* another process, later: nothing but the file */
    memset(log, 0, n * 32);
    f = fopen(path, "rb");
    if (!f || fread(log, 32, n, f) != n) { fprintf(stderr, "cannot read %s\n", path); return 1; }
    fclose(f);
    uint64_t bad_pos = 0;
    if ((rc = imt_itree_load_values(cold, log, n, &bad_pos, IMT_FMT_CANONICAL))) {
        fprintf(stderr, "load_values: %s\n", imt_last_error(ctx));
        return 1;
    }
    if ((rc = imt_itree_root(cold, root_b, IMT_FMT_CANONICAL))) { fprintf(stderr, "%s\n", imt_last_error(ctx)); return 1; }
    printf("cold start: %llu leaves, root %s\n", (unsigned long long)imt_itree_size(cold), show(root_b, hex_b));
    int bad = memcmp(root_a, root_b, 32) != 0;
    printf("the two roots %s\n", bad ? "DIFFER" : "are equal");
    if (argc > 1) {
        const int off = strcmp(argv[1], hex_b) != 0;
        printf("cold-start root %s\n", off ? "DIFFERS from the expected one" : "equals the expected one");
        bad |= off;
    }
    /* a log that inserting one by one would not get through: value 7 again at the end */
    memcpy(log + n * 32, log + 7 * 32, 32);
    rc = imt_itree_load_values(cold, log, n + 1, &bad_pos, IMT_FMT_CANONICAL);
    unsigned char root_c[32];
    const int kept = rc == IMT_ERR_VALUE && bad_pos == n && !imt_itree_root(cold, root_c, IMT_FMT_CANONICAL) &&
                     !memcmp(root_b, root_c, 32) && imt_itree_size(cold) == size;
    printf("a log with a repeated value: %s\n", kept ? "refused at the repeat, the tree as it was" : "NOT refused as it should be");
    free(log);
    imt_itree_free(cold);
    imt_itree_free(follower);
    imt_ctx_destroy(ctx);
    remove(path);
    return bad || !kept;
}
