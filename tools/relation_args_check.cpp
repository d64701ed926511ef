// Stand-alone check of the argument validation of mkb_rel_scores, mkb_rel_rank and mkb_rel_topk: every call below must be refused
// with MKB_ERR_INVALID (rows too long for the kernel: MKB_ERR_UNSUPPORTED) before anything is launched (it runs on a machine
// without a GPU), and the error text must be set; B == 0 is a valid call that launches nothing.
// Built with the host sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       tools/relation_args_check.cpp mkb_amd/csrc/score_relation.hip mkb_amd/csrc/core.hip -o /tmp/relation_args_check && /tmp/relation_args_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/mkb_hip.h"

static int failures = 0;

static void expect(int want, int rc, const char *what) {
    const char *msg = mkb_last_error();
    if (rc != want || (want != MKB_OK && (!msg || strlen(msg) == 0))) {
        printf("FAIL %s: status %d (wanted %d), message '%s'\n", what, rc, want, msg ? msg : "(null)");
        ++failures;
    }
}
static void expect_invalid(int rc, const char *what) { expect(MKB_ERR_INVALID, rc, what); }

int main() {
    // host arrays standing in for device buffers: validation must not read or write them
    static float ent[100 * 16], rel[3 * 8], modulus[1], scores[4 * 8];
    alignas(256) static unsigned char ws[4096];
    int64_t sample[12] = {0}, keys[4] = {0}, rel_ids[5] = {0}, rank[4], ids[4 * 8];
    for (int i = 0; i < 32; ++i) scores[i] = 42.f, ids[i] = 42;
    for (int i = 0; i < 4; ++i) rank[i] = 42;
    const mkb_tables_t tb = {MKB_ROTATE, 8, 100, 3, 16, 8, ent, rel, modulus, 6.f, 1.f};
    mkb_tables_t bad_model = tb, mismatch = tb, long_rows = tb;
    bad_model.model = 99;
    mismatch.entity_dim = 8;
    long_rows.model = MKB_TRANSE; long_rows.hidden_dim = 4096; long_rows.entity_dim = long_rows.relation_dim = 4096;
    const int64_t big = (int64_t)1 << 31;

    expect_invalid(mkb_rel_scores(nullptr, sample, 4, nullptr, 3, scores, 3, nullptr), "scores: null tables");
    expect_invalid(mkb_rel_scores(&bad_model, sample, 4, nullptr, 3, scores, 3, nullptr), "scores: unknown model");
    expect_invalid(mkb_rel_scores(&mismatch, sample, 4, nullptr, 3, scores, 3, nullptr), "scores: row length / model mismatch");
    expect_invalid(mkb_rel_scores(&tb, nullptr, 4, nullptr, 3, scores, 3, nullptr), "scores: null sample");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, nullptr, 3, nullptr, 3, nullptr), "scores: null scores");
    expect_invalid(mkb_rel_scores(&tb, sample, -1, nullptr, 3, scores, 3, nullptr), "scores: negative B");
    expect_invalid(mkb_rel_scores(&tb, sample, big, nullptr, 3, scores, 3, nullptr), "scores: B > 2^31 - 1");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, nullptr, 3, scores, 2, nullptr), "scores: ld < n_rel");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, rel_ids, 5, scores, 4, nullptr), "scores: ld < n_rel with a list");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, rel_ids, 0, scores, 3, nullptr), "scores: n_rel = 0");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, rel_ids, -2, scores, 3, nullptr), "scores: negative n_rel");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, rel_ids, big, scores, big, nullptr), "scores: n_rel > 2^31 - 1");
    expect_invalid(mkb_rel_scores(&tb, sample, 4, nullptr, 2, scores, 3, nullptr), "scores: null rel_ids, n_rel != n_relation");
    expect(MKB_ERR_UNSUPPORTED, mkb_rel_scores(&long_rows, sample, 4, nullptr, 3, scores, 3, nullptr), "scores: rows too long");
    expect(MKB_OK, mkb_rel_scores(&tb, sample, 0, nullptr, 3, scores, 3, nullptr), "scores: B = 0");

    const int64_t need = mkb_rel_rank_workspace_bytes(&tb, 4);
    if (need <= 0 || need > (int64_t)sizeof ws || mkb_rel_topk_workspace_bytes(&tb, 4, 8) != need) {
        printf("FAIL workspace size %lld\n", (long long)need);
        ++failures;
    }
    if (mkb_rel_rank_workspace_bytes(nullptr, 4) || mkb_rel_rank_workspace_bytes(&tb, 0) || mkb_rel_rank_workspace_bytes(&tb, -1) ||
        mkb_rel_rank_workspace_bytes(&tb, big) || mkb_rel_topk_workspace_bytes(&tb, 4, 0) || mkb_rel_topk_workspace_bytes(&tb, 4, 1025) ||
        mkb_rel_topk_workspace_bytes(nullptr, 4, 8) || mkb_rel_topk_workspace_bytes(&tb, 0, 8)) {
        printf("FAIL a workspace function answered a bad argument with a size\n");
        ++failures;
    }

    expect_invalid(mkb_rel_rank(nullptr, sample, 4, keys, 4, rank, scores, ws, need, nullptr), "rank: null tables");
    expect_invalid(mkb_rel_rank(&bad_model, sample, 4, keys, 4, rank, scores, ws, need, nullptr), "rank: unknown model");
    expect_invalid(mkb_rel_rank(&tb, nullptr, 4, keys, 4, rank, scores, ws, need, nullptr), "rank: null sample");
    expect_invalid(mkb_rel_rank(&tb, sample, 4, keys, 4, nullptr, scores, ws, need, nullptr), "rank: null rank");
    expect_invalid(mkb_rel_rank(&tb, sample, -1, keys, 4, rank, scores, ws, need, nullptr), "rank: negative B");
    expect_invalid(mkb_rel_rank(&tb, sample, big, keys, 4, rank, scores, ws, need, nullptr), "rank: B > 2^31 - 1");
    expect_invalid(mkb_rel_rank(&tb, sample, 4, nullptr, 4, rank, scores, ws, need, nullptr), "rank: n_true > 0 with null keys");
    expect_invalid(mkb_rel_rank(&tb, sample, 4, keys, -1, rank, scores, ws, need, nullptr), "rank: negative n_true");
    expect_invalid(mkb_rel_rank(&tb, sample, 4, keys, 4, rank, scores, nullptr, need, nullptr), "rank: null workspace");
    expect_invalid(mkb_rel_rank(&tb, sample, 4, keys, 4, rank, scores, ws, need - 1, nullptr), "rank: short workspace");
    expect_invalid(mkb_rel_rank(&tb, sample, 4, keys, 4, rank, scores, ws + 16, need, nullptr), "rank: misaligned workspace");
    expect(MKB_ERR_UNSUPPORTED, mkb_rel_rank(&long_rows, sample, 4, keys, 4, rank, nullptr, ws, need, nullptr), "rank: rows too long");
    expect(MKB_OK, mkb_rel_rank(&tb, sample, 0, nullptr, 0, rank, nullptr, nullptr, 0, nullptr), "rank: B = 0");

    expect_invalid(mkb_rel_topk(nullptr, sample, 4, keys, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: null tables");
    expect_invalid(mkb_rel_topk(&bad_model, sample, 4, keys, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: unknown model");
    expect_invalid(mkb_rel_topk(&tb, nullptr, 4, keys, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: null sample");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, 0, nullptr, scores, ws, need, nullptr), "topk: null ids");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, 0, ids, nullptr, ws, need, nullptr), "topk: null scores");
    expect_invalid(mkb_rel_topk(&tb, sample, -1, keys, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: negative B");
    expect_invalid(mkb_rel_topk(&tb, sample, big, keys, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: B > 2^31 - 1");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 0, 0, ids, scores, ws, need, nullptr), "topk: k = 0");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, MKB_TOPK_MAX_K + 1, 0, ids, scores, ws, need, nullptr), "topk: k too large");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, -3, 0, ids, scores, ws, need, nullptr), "topk: negative k");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, 2, ids, scores, ws, need, nullptr), "topk: unknown flag");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, -1, ids, scores, ws, need, nullptr), "topk: negative flags");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, nullptr, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: n_true > 0 with null keys");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, 0, ids, scores, nullptr, need, nullptr), "topk: null workspace");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, 0, ids, scores, ws, need - 1, nullptr), "topk: short workspace");
    expect_invalid(mkb_rel_topk(&tb, sample, 4, keys, 4, 2, 0, ids, scores, ws + 16, need, nullptr), "topk: misaligned workspace");
    expect(MKB_ERR_UNSUPPORTED, mkb_rel_topk(&long_rows, sample, 4, keys, 4, 2, 0, ids, scores, ws, need, nullptr), "topk: rows too long");
    expect(MKB_OK, mkb_rel_topk(&tb, sample, 0, nullptr, 0, 2, MKB_TOPK_KEEP_TARGET, ids, scores, nullptr, 0, nullptr), "topk: B = 0");

    for (int i = 0; i < 32; ++i)
        if (scores[i] != 42.f || ids[i] != 42 || rank[i % 4] != 42) {
            printf("FAIL: a refused call wrote its output\n");
            ++failures;
            break;
        }
    printf(failures ? "%d check(s) failed\n" : "all argument checks passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
