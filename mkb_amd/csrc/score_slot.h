// What score_relation.hip, the owner of the slot forward (slot_score_kernel), offers score_cand.hip: the launch and the refusal
// of rows too long for it.  256 lanes, 4 waves per workgroup in every slot kernel.
#pragma once
#include "common.h"

namespace mkb {

constexpr int kSlotBlock = 256, kSlotWaves = kSlotBlock / 64;

// MKB_ERR_UNSUPPORTED where the h row, the t row and one query row per wave do not fit the score kernel's 64 KB of LDS
int slot_rows_check(const mkb_tables_t *tb);

// the scores of n_cand candidates per row in the relation slot (vary_head: the head slot).  cand: row i's list is cand + i *
// cand_stride (stride 0: one list for the whole batch); null = the ids 0 .. n_cand - 1
int launch_slot_scores(const mkb_tables_t *tb, const int64_t *sample, int64_t B, const int64_t *cand, int64_t cand_stride, int64_t n_cand,
                       bool vary_head, float *scores, int64_t ld, hipStream_t st);

}  // namespace mkb
