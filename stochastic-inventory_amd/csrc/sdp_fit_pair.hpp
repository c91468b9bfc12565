// sdp_fit_pair.hpp -- the record batch_fit_ss_kernel (sdp_fitss.hpp) reads per (instance, period), on its own so that a unit which
// only FILLS such records (sdpgpu_staffbatch.hip) does not pull in the backorder batch's kernels.
#pragma once
#include <cstdint>

namespace sdp {

// the reachable slice of one (instance, period): rows lo .. lo + n - 1 of its policy row
struct FitPair {
  int64_t pol_off;  // of the (instance, period)'s policy row in the batch's arena
  double x_min;     // inventory of the row's state 0
  double maxq;      // the instance's order limit (a staff batch: the caller's limit)
  int32_t lo, n;    // the reachable states lo .. lo + n - 1
};

}  // namespace sdp
