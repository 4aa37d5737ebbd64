// What the launchers (through sea_common.h) and the host-only selection plans (upsample_plan.h) share: the argument-error
// code and the grid sizes of the memory-bound grid-stride launches.  Integers only, no HIP header.
#pragma once
#include <stdint.h>

#define SEA_ERR_ARG 1  // == hipErrorInvalidValue

namespace sea {

constexpr int kMaxGridX = 256 * 8; // memory-bound launches: <= 8 blocks per CU, grid-stride beyond

static inline int grid_for(int64_t work_items, int block) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > kMaxGridX) g = kMaxGridX;
  return (int)g;
}

// a multiple of 8 blocks: what a kernel that walks its index space through xcd_range() (sea_common.h) needs
static inline int grid_for_xcd(int64_t work_items, int block) {
  const int g = grid_for(work_items, block);
  return (g + 7) / 8 * 8;
}

}  // namespace sea
