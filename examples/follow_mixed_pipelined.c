/* follow_mixed_pipelined.c -- follow_pipelined.c for a chain whose blocks hold verify_non_inclusion transactions, in plain C
 * against include/imt.h.  Every fourth transaction of a block only asserts that a value is absent at that point of the
 * block (IMT_OP_READ), the others insert a nullifier (IMT_OP_INSERT); only the ordered walk decides whether the READs hold,
 * so the follower cannot hand the INSERT values to imt_itree_apply_pipelined.  imt_itree_apply_mixed_pipelined walks the
 * block and returns when it has passed its checks; the hashing of up to four blocks overlaps on the GPU, and every block
 * delivers its own root into a row of page-locked memory the GPU addresses.  One imt_ctx_sync() later all roots are there
 * and are compared with the ones the chain announced (here: a second tree fed block by block with imt_itree_apply_mixed).
 * Ten blocks of 64 transactions into a depth-32 tree; block 6 holds READs only and must report the root of block 5.  A READ
 * asks for the value its neighbour in the block inserts later, or for one no block ever inserts.  With an argument (64 hex
 * digits, most significant first) the last root is compared with it and the exit status says whether they are equal.
 * Build:
 *   gcc -std=c11 -I include examples/follow_mixed_pipelined.c -L indexed-merkle-tree-halo2_amd/csrc -limt_hip \
 *       -o follow_mixed_pipelined
 */
#include <stdio.h>
#include <string.h>
#include "imt.h"

#define BLOCKS 10
#define PER_BLOCK 64
#define DEPTH 32
#define READS_ONLY 6

static void fail(imt_ctx *ctx, const char *what) {
    fprintf(stderr, "%s: %s\n", what, imt_last_error(ctx));
}

/* the value of transaction i of block j: an INSERT's nullifier -- distinct, non-zero, in no order; a READ at i = 4k + 1
 * asks for the nullifier transaction i + 1 inserts, a READ of the block of READs for a value of its own */
static uint64_t tx_value(int j, int i, int is_read) {
    const uint64_t q = (uint64_t)(PER_BLOCK * j + i + 1 + (is_read && j != READS_ONLY));
    return 1 + 7919023757ULL * q % ((1ULL << 61) - 1);
}

int main(int argc, char **argv) {
    imt_ctx *ctx = NULL;
    imt_itree *tree = NULL, *chain = NULL;
    void *mem = NULL;
    int rc = imt_ctx_create(0, &ctx);
    if (rc) { fprintf(stderr, "imt_ctx_create: %d (no GPU?)\n", rc); return 1; }
    if (imt_itree_new(ctx, DEPTH, 1024, &tree) || imt_itree_new(ctx, DEPTH, 1024, &chain)) { fail(ctx, "imt_itree_new"); return 1; }
    /* every block's values, every block's root, then every block's op bytes: rows of 32 bytes the GPU addresses */
    const size_t rows = (size_t)BLOCKS * (PER_BLOCK + 1), bytes = rows * 32 + (size_t)BLOCKS * PER_BLOCK;
    if (imt_host_alloc(ctx, bytes, &mem)) { fail(ctx, "imt_host_alloc"); return 1; }
    unsigned char (*vals)[32] = mem, (*root)[32] = vals + BLOCKS * PER_BLOCK;
    uint8_t *op = (uint8_t *)mem + rows * 32;
    memset(mem, 0, bytes);
    for (int j = 0; j < BLOCKS; j++)
        for (int i = 0; i < PER_BLOCK; i++) {
            const int is_read = j == READS_ONLY || i % 4 == 1;
            const uint64_t v = tx_value(j, i, is_read);
            op[PER_BLOCK * j + i] = is_read ? IMT_OP_READ : IMT_OP_INSERT;
            for (int k = 0; k < 8; k++) vals[PER_BLOCK * j + i][k] = (unsigned char)(v >> (8 * k));
        }

    /* what the block headers say: the chain's own tree, one block at a time */
    unsigned char announced[BLOCKS][32];
    uint64_t inserted = 0, total = 0;
    for (int j = 0; j < BLOCKS; j++) {
        if (imt_itree_apply_mixed(chain, vals[PER_BLOCK * j], op + PER_BLOCK * j, PER_BLOCK, announced[j], &inserted, NULL,
                                  IMT_FMT_CANONICAL)) {
            fail(ctx, "imt_itree_apply_mixed");
            return 1;
        }
        total += inserted;
    }

    /* the follower: every block enqueued behind the one before, nothing waited for but each block's checks -- after which
     * the block's values and op bytes are the caller's again */
    uint64_t followed = 0, bad_op = 0;
    for (int j = 0; j < BLOCKS; j++) {
        if (imt_itree_apply_mixed_pipelined(tree, vals[PER_BLOCK * j], op + PER_BLOCK * j, PER_BLOCK, root[j], &inserted, &bad_op,
                                            IMT_FMT_CANONICAL | IMT_DEVICE_PTRS)) {
            fail(ctx, "imt_itree_apply_mixed_pipelined");   /* a refused block: the blocks before it are in the tree */
            return 1;
        }
        followed += inserted;
        memset(vals[PER_BLOCK * j], 0xff, (size_t)PER_BLOCK * 32);
        memset(op + PER_BLOCK * j, 0xff, PER_BLOCK);
    }
    if (imt_ctx_sync(ctx)) { fail(ctx, "imt_ctx_sync"); return 1; }

    char hex[65] = {0};
    int bad = followed != total || imt_itree_size(tree) != total + 1;
    printf("%llu insertions in %d blocks\n", (unsigned long long)followed, BLOCKS);
    for (int j = 0; j < BLOCKS; j++) {
        for (int k = 0; k < 32; k++) sprintf(hex + 2 * k, "%02x", root[j][31 - k]);
        const int same = memcmp(root[j], announced[j], 32) == 0;
        printf("block %d: root %s %s\n", j, hex, same ? "as announced" : "NOT the announced one");
        bad |= !same;
    }
    if (memcmp(root[READS_ONLY], root[READS_ONLY - 1], 32) != 0) {
        printf("the block of READs changed the root\n");
        bad = 1;
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
