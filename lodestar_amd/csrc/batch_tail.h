// Shapes of the batch-first tail (dev_batch.batch_tail),
// shared by the kernels' launchers (bgv_kernels.hip launch_batch_sig,
// bgv_tail.hip launch_batch_chain), the allocation (bgv_api.hip work_alloc)
// and the host check (tests/native/hostcheck_batch_tail.cpp).
//
// Both trees run level by level, level L reading n values and writing
// ceil(n / FAN) of them, ping-ponging between two regions of one buffer:
// region 0 holds level 0's output (and levels 2, 4, ...), region 1 level 1's
// (and 3, 5, ...), so a level never writes what it reads.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bgv {

// fan-in of the Fp12 folds (k_fold, k_step_fold): a fan-in of 8 keeps the chain of sequential Fp12 products short
constexpr uint32_t FOLD_FAN = 8;
// fan-in of the window-sum tree over the jobs (k_win_fold): 3 G2 additions per level on the chain
constexpr uint32_t WIN_FAN = 4;

constexpr uint32_t tail_groups(uint32_t n, uint32_t fan) { return (n + fan - 1u) / fan; }
// start of region 1, and the whole buffer, in values per (step | window)
constexpr size_t tail_region1(uint32_t n, uint32_t fan) { return tail_groups(n, fan); }
constexpr size_t tail_entries(uint32_t n, uint32_t fan) { return (size_t)tail_groups(n, fan) + tail_groups(tail_groups(n, fan), fan); }

}  // namespace bgv
