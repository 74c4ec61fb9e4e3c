/* follow_pipelined.c -- a follower that applies small blocks and checks every block's root, in plain C against
 * include/imt.h.  follow_chain.c applies a block, waits, compares, applies the next; here the blocks are enqueued one
 * after the other with imt_itree_apply_pipelined -- each call returns when the block's values are checked, the hashing of
 * up to four blocks overlaps on the GPU -- and every block still delivers its own root, into a row of page-locked memory
 * the GPU addresses.  One imt_ctx_sync() later all roots are there and are compared with the ones the chain announced
 * (here: a second tree fed block by block with imt_itree_apply_batch).  Ten blocks of 64 values into a depth-32 tree,
 * follow_chain.c's stream.  With an argument (64 hex digits, most significant first) the last root is compared with it
 * and the exit status says whether they are equal.  Build:
 *   gcc -std=c11 -I include examples/follow_pipelined.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip -o follow_pipelined
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define PER_BLOCK 64
#define DEPTH 32

static void fail(imt_ctx *ctx, const char *what) {
    fprintf(stderr, "%s: %s\n", what, imt_last_error(ctx));
}

int main(int argc, char **argv) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL, *chain = NULL;
    void *mem = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if (imt_itree_new(ctx, DEPTH, 1024, &tree) || imt_itree_new(ctx, DEPTH, 1024, &chain)) { fail(ctx, "imt_itree_new"); return 1; }
    /* every block's values, then every block's root: rows of 32 bytes, 16-byte aligned, addressed by the GPU */
    if (imt_host_alloc(ctx, (size_t)BLOCKS * (PER_BLOCK + 1) * 32, &mem)) { fail(ctx, "imt_host_alloc"); return 1; }
    unsigned char (*vals)[32] = mem, (*root)[32] = vals + BLOCKS * PER_BLOCK;
    memset(mem, 0, (size_t)BLOCKS * (PER_BLOCK + 1) * 32);
    for (int j = 0; j < BLOCKS; j++)
        for (int i = 0; i < PER_BLOCK; i++) {         /* a block's nullifiers: distinct, non-zero, in no order */
            const uint64_t v = 1 + 7919023757ULL * (uint64_t)(PER_BLOCK * j + i + 1) % ((1ULL << 61) - 1);
            for (int k = 0; k < 8; k++) vals[PER_BLOCK * j + i][k] = (unsigned char)(v >> (8 * k));
        }

    /* what the block headers say: the chain's own tree, one block at a time */
    unsigned char announced[BLOCKS][32];
    for (int j = 0; j < BLOCKS; j++)
        if (imt_itree_apply_batch(chain, vals[PER_BLOCK * j], PER_BLOCK, announced[j], IMT_FMT_CANONICAL)) {
            fail(ctx, "imt_itree_apply_batch");
            return 1;
        }

    /* the follower: every block enqueued behind the one before, nothing waited for but each block's value check */
    for (int j = 0; j < BLOCKS; j++)
        if (imt_itree_apply_pipelined(tree, vals[PER_BLOCK * j], PER_BLOCK, root[j], IMT_FMT_CANONICAL | IMT_DEVICE_PTRS)) {
            fail(ctx, "imt_itree_apply_pipelined");       /* a refused block: the blocks before it are in the tree */
            return 1;
        }
    if (imt_ctx_sync(ctx)) { fail(ctx, "imt_ctx_sync"); return 1; }

    char hex[65] = {0};
    int bad = 0;
    for (int j = 0; j < BLOCKS; j++) {
        for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[j][31 - k]);
        const int same = memcmp(root[j], announced[j], 32) == 0;
        printf("block %d: root %s %s\n", j, hex, same ? "as announced" : "NOT the announced one");
        bad |= !same;
    }
    if (argc > 1) {
        const int differs = strcmp(argv[1], hex) != 0;
        printf("final root %s\n", differs ? "DIFFERS from the expected one" : "equals the expected one");
        bad |= differs;
    }
    imt_host_free(ctx, mem);
    imt_itree_free(tree);
    imt_itree_free(chain);
    imt_ctx_destroy(ctx);
    return bad;
}
