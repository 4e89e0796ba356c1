// rub_mimo_amd/csrc/est_common.hpp -- what more than one of the channel estimation kernel
// files use (codes_kernels.hip, est_kernels.hip, ls_kernels.hip; weights_kernels.hip needs
// none of it). A helper with one user lives in that file.
#pragma once

#include "kernels.hpp"

namespace mimo {

constexpr int kEstT = 256;

MIMO_DEV uint32_t key_index(unsigned long long k) {
  return k ? (0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull)) : 0u;
}

constexpr int kLsRotCodes = 256;   // CFO code rotations tabled in LDS

}  // namespace mimo
