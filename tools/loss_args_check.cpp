// Stand-alone check of the argument validation of mkb_ns_loss: every call below must be refused with MKB_ERR_INVALID before
// anything is launched (it runs on a machine without a GPU), the error text must be set, and no output may be written.
// Built with the host sanitizers, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       tools/loss_args_check.cpp mkb_amd/csrc/ns_loss.hip mkb_amd/csrc/core.hip -o /tmp/loss_args_check && /tmp/loss_args_check
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../include/mkb_hip.h"

static int failures = 0;

static void expect_invalid(int rc, const char *what) {
    const char *msg = mkb_last_error();
    if (rc != MKB_ERR_INVALID || !msg || strlen(msg) == 0) {
        printf("FAIL %s: status %d (wanted %d), message '%s'\n", what, rc, MKB_ERR_INVALID, msg ? msg : "(null)");
        ++failures;
    }
}

int main() {
    // host arrays standing in for device buffers: validation must not read or write them
    static float pos[4], neg[12], w[4], wsum[1], loss[1], dpos[4], dneg[12], scratch[5];
    static uint16_t cnt[12];
    loss[0] = 42.f;
    for (int i = 0; i < 4; ++i) dpos[i] = 42.f;
    for (int i = 0; i < 12; ++i) dneg[i] = 42.f;
    for (int i = 0; i < 5; ++i) scratch[i] = 42.f;
    const int64_t big = (int64_t)1 << 31;
    const float nan = nanf(""), inf = INFINITY;
    const int M = MKB_LOSS_MARGIN, P = MKB_LOSS_PAIR_LOGISTIC, S = MKB_LOSS_SOFTMAX;

    expect_invalid(mkb_ns_loss(M, nullptr, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "null pos");
    expect_invalid(mkb_ns_loss(M, pos, nullptr, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "null neg");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, nullptr, dpos, dneg, scratch, nullptr), "null loss");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, nullptr, dneg, scratch, nullptr), "null dpos");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, dpos, nullptr, scratch, nullptr), "null dneg");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, dpos, dneg, nullptr, nullptr), "null scratch");
    expect_invalid(mkb_ns_loss(P, nullptr, neg, nullptr, nullptr, 4, 3, 1.f, 0.f, nullptr, loss, dpos, dneg, scratch, nullptr),
                   "null pos without the optional arrays");
    expect_invalid(mkb_ns_loss(3, pos, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "kind 3");
    expect_invalid(mkb_ns_loss(-1, pos, neg, w, cnt, 4, 3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "kind -1");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 0, 3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "B = 0");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, -4, 3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "negative B");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 0, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "K = 0");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, -3, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "negative K");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, big, 1, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "B > 2^31 - 1");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 1, big, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "K > 2^31 - 1");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 1 << 16, 1 << 15, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "B * K = 2^31");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, INT64_MAX, INT64_MAX, 1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr),
                   "B * K overflows int64");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 3, 1.f, -0.5f, wsum, loss, dpos, dneg, scratch, nullptr), "alpha < 0");
    expect_invalid(mkb_ns_loss(P, pos, neg, w, cnt, 4, 3, 1.f, nan, wsum, loss, dpos, dneg, scratch, nullptr), "alpha NaN");
    expect_invalid(mkb_ns_loss(P, pos, neg, w, cnt, 4, 3, 1.f, inf, wsum, loss, dpos, dneg, scratch, nullptr), "alpha inf");
    expect_invalid(mkb_ns_loss(M, pos, neg, w, cnt, 4, 3, nan, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "margin NaN");
    expect_invalid(mkb_ns_loss(P, pos, neg, w, cnt, 4, 3, -inf, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "margin -inf");
    expect_invalid(mkb_ns_loss(S, pos, neg, w, cnt, 4, 3, 0.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "T = 0");
    expect_invalid(mkb_ns_loss(S, pos, neg, w, cnt, 4, 3, -1.f, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "T < 0");
    expect_invalid(mkb_ns_loss(S, pos, neg, w, cnt, 4, 3, inf, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "T inf");
    expect_invalid(mkb_ns_loss(S, pos, neg, w, cnt, 4, 3, nan, 0.f, wsum, loss, dpos, dneg, scratch, nullptr), "T NaN");

    bool wrote = loss[0] != 42.f;
    for (int i = 0; i < 4; ++i) wrote |= dpos[i] != 42.f;
    for (int i = 0; i < 12; ++i) wrote |= dneg[i] != 42.f;
    for (int i = 0; i < 5; ++i) wrote |= scratch[i] != 42.f;
    if (wrote) {
        printf("FAIL: a refused call wrote its output\n");
        ++failures;
    }
    printf(failures ? "%d check(s) failed\n" : "all argument checks passed (%d failures)\n", failures);
    return failures ? 1 : 0;
}
