// Stand-alone check of the argument validation of mkb_relation_fanout and mkb_rank_metrics: every call below must be refused
// with MKB_ERR_INVALID before anything is launched (it runs on a machine without a GPU), and the error text must be set.
// Built with the host sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       tools/metrics_args_check.cpp mkb_amd/csrc/metrics.hip mkb_amd/csrc/core.hip -o /tmp/metrics_args_check && /tmp/metrics_args_check
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/mkb_hip.h"

static int failures = 0;

static void expect_invalid(int rc, const char *what) {
    const char *msg = mkb_last_error();
    if (rc != MKB_ERR_INVALID || !msg || strlen(msg) == 0) {
        printf("FAIL %s: status %d, message '%s'\n", what, rc, msg ? msg : "(null)");
        ++failures;
    }
}

int main() {
    // host arrays standing in for device buffers: validation must not read or write them
    int64_t triples[12] = {0}, keys[4] = {0}, counts[15], ranks[4] = {1, 1, 1, 1};
    int32_t table[3] = {0, 1, -1};
    double rr[4];
    for (int i = 0; i < 15; ++i) counts[i] = 42;
    const int64_t big = INT64_MAX / 2;

    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, 4, 0, 3, counts, nullptr), "fanout: no entities");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, 4, -7, 3, counts, nullptr), "fanout: negative entities");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, 4, 10, 0, counts, nullptr), "fanout: no relations");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, 4, 10, -1, counts, nullptr), "fanout: negative relations");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, 4, 10, (int64_t)1 << 31, counts, nullptr), "fanout: too many relations");
    expect_invalid(mkb_relation_fanout(triples, -1, keys, 4, keys, 4, 10, 3, counts, nullptr), "fanout: negative n");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, -1, keys, 4, 10, 3, counts, nullptr), "fanout: negative n_head");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, INT64_MIN, 10, 3, counts, nullptr), "fanout: negative n_tail");
    expect_invalid(mkb_relation_fanout(triples, big, keys, big, keys, big, 10, 3, counts, nullptr), "fanout: counts that overflow");
    expect_invalid(mkb_relation_fanout(nullptr, 4, keys, 4, keys, 4, 10, 3, counts, nullptr), "fanout: null triples");
    expect_invalid(mkb_relation_fanout(triples, 4, nullptr, 4, keys, 4, 10, 3, counts, nullptr), "fanout: null head keys");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, nullptr, 4, 10, 3, counts, nullptr), "fanout: null tail keys");
    expect_invalid(mkb_relation_fanout(triples, 4, keys, 4, keys, 4, 10, 3, nullptr, nullptr), "fanout: null counts");
    expect_invalid(mkb_relation_fanout(nullptr, 0, nullptr, 0, nullptr, 0, 10, 3, nullptr, nullptr), "fanout: null counts, nothing to count");

    expect_invalid(mkb_rank_metrics(ranks, triples, 4, table, 0, 4, counts, rr, nullptr), "metrics: no relations");
    expect_invalid(mkb_rank_metrics(ranks, triples, 4, table, -3, 4, counts, rr, nullptr), "metrics: negative relations");
    expect_invalid(mkb_rank_metrics(ranks, triples, 4, table, 3, 0, counts, rr, nullptr), "metrics: no groups");
    expect_invalid(mkb_rank_metrics(ranks, triples, 4, table, 3, INT32_MIN, counts, rr, nullptr), "metrics: negative groups");
    expect_invalid(mkb_rank_metrics(ranks, triples, -1, table, 3, 3, counts, rr, nullptr), "metrics: negative n");
    expect_invalid(mkb_rank_metrics(ranks, triples, INT64_MAX, table, 3, 3, counts, rr, nullptr), "metrics: n that overflows 3 n");
    expect_invalid(mkb_rank_metrics(nullptr, triples, 4, table, 3, 3, counts, rr, nullptr), "metrics: null ranks");
    expect_invalid(mkb_rank_metrics(ranks, nullptr, 4, table, 3, 3, counts, rr, nullptr), "metrics: null sample");
    expect_invalid(mkb_rank_metrics(ranks, triples, 4, nullptr, 3, 3, counts, rr, nullptr), "metrics: null table");
    expect_invalid(mkb_rank_metrics(ranks, triples, 4, table, 3, 3, nullptr, rr, nullptr), "metrics: null counts");
    expect_invalid(mkb_rank_metrics(ranks, triples, 4, table, 3, 3, counts, nullptr, nullptr), "metrics: null rr_sum");
    expect_invalid(mkb_rank_metrics(nullptr, nullptr, 0, nullptr, 3, 3, counts, rr, nullptr), "metrics: null table, no items");

    for (int i = 0; i < 15; ++i)
        if (counts[i] != 42) {
            printf("FAIL: a refused call wrote its output\n");
            ++failures;
            break;
        }
    printf(failures ? "%d check(s) failed\n" : "all argument checks passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
