// sdp_staff_batch.hpp -- the separable mode of the STAFF family (sdp_staff_sep.hpp) for a BATCH of instances of one shape:
// period t of ALL instances in two launches (sdpgpu_staffbatch.hip), every instance's tables bit for bit those of its own
// separable handle.
//
// The instances of a batch share T, the hire limit, the bounds and iniStaffNum, hence every period's staff range, its levels
// and the bounds of the next staff number: those travel in the kernel argument (StaffBatchLaunch).  What an instance owns --
// fixCost, unitVariCost, salary, unitPenalty, minStaffNum[t], the level table of the period and where its rows lie in the
// arenas -- is a record in device memory (StaffBatchInst, [t][i]), read through wave-uniform addresses.
//
// G launch (staff_batch_g_kernel<R, U, FUTURE>): a wave is 64 consecutive levels of a BLOCK of R instances that integrate
// over the same table in this period.  The walk is staff_g_kernel's: the wave's step counter, the table row of a step a scalar
// address plus the lane's level offset, the staff left y - j one subtraction from a scalar, lanes with a shorter row not taking
// the steps past its end, reads ahead of the longest row folded onto its last step.  The probability p_row(j), the staff
// left, the index into V_{t+1} and the weight chain ps are formed ONCE for the R instances (P_t(y) depends on the table only);
// every instance keeps its own w, its own V read and its own chain `g += p * w; g += p * V` in ascending j, without FMA --
// the operations and the order of its handle's lane.  U steps are read ahead in two register sets, as in the handle's kernel;
// with R value streams a set holds U (1 + R) doubles, so U shrinks as R grows (kStaffBatchU*, chosen from the compiled
// kernels' register use: profiles/staff_batch_resources.txt).  The last block of a group may be short: its spare slots repeat
// the last instance (inst[r] == inst[r - 1]) and store nothing, as lanes past the last level already do.
//
// Scan launch (staff_batch_min_kernel): staff_sep_min_kernel with the instance taken from the workgroup index and the
// instance's own K, v and rows.
#pragma once
#include "sdp_device.hpp"

namespace sdp {

// the instance block of the G launch where a (period, table) group holds at least that many instances, else 1.
// Measured on WorkforceTesting.main's 216 instances (tools/staff_batch_rows.py --batch-only --lib <build>, 7 samples, MI355X;
// DESIGN 9): R = 1 11.0 ms whatever U (4 / 8 / 16: 10.97 / 11.10 / 11.02 at 71 / 128 / 146 VGPRs), R = 2 9.66 (U = 8) and 9.80
// (U = 4), R = 4 9.58 / 9.32 / 9.31 ms for U = 2 / 4 / 8 at 108 / 112 / 192 VGPRs.  Kept: R = 4 with U = 4 (four waves a SIMD;
// U = 8 is no faster at two), and U = 4 for single instances (seven waves).  -DSDP_STAFF_BATCH_R / _U1 / _UR build the others.
#ifndef SDP_STAFF_BATCH_R
#define SDP_STAFF_BATCH_R 4
#endif
#ifndef SDP_STAFF_BATCH_U1
#define SDP_STAFF_BATCH_U1 4
#endif
#ifndef SDP_STAFF_BATCH_UR
#define SDP_STAFF_BATCH_UR 4
#endif
constexpr int kStaffBatchR = SDP_STAFF_BATCH_R;
constexpr int kStaffBatchU1 = SDP_STAFF_BATCH_U1;  // steps read ahead per register set, R = 1
constexpr int kStaffBatchUR = SDP_STAFF_BATCH_UR;  // ... R = kStaffBatchR
static_assert(kStaffBatchR == 1 || kStaffBatchR == 2 || kStaffBatchR == 4, "instantiated blocks: 1, 2, 4");

struct StaffBatchInst {   // one per (period, instance)
  double K, v, salary, pen;
  int32_t min_staff;
  int32_t table;          // id in the pool
  int64_t v_cur_off, v_next_off;  // elements into the value arena (v_next_off unused in the last period)
  int64_t pol_off;        // elements into the policy arena
};

struct StaffBatchTable {  // one per pool table: the transposed table pT[j * n_rows + y], zero behind a row's length
  const double* pT;
  const int32_t* row_len;
  int32_t n_rows, max_j;
};

struct StaffBatchLaunch {  // common to the batch
  int32_t n_actions;
  int32_t y0;              // staff number of state index 0 = lowest level of the period
  int32_t n_levels;        // states + actions - 1
  int32_t n_states;
  int32_t next_x_lo, nn_lo, nn_hi;  // as StaffParams (sdp_staff.hpp)
  int32_t g_blocks;        // waves of 64 levels per instance block
  int32_t tiles;           // workgroups of 64 states per instance
  int64_t lev_stride;      // elements between two rows of the arena gp[i][2][lev_stride]
};

template <int R, int U, bool FUTURE>
__global__ __launch_bounds__(64) void staff_batch_g_kernel(StaffBatchLaunch L, const StaffBatchInst* __restrict__ inst,
                                                           const StaffBatchTable* __restrict__ tabs,
                                                           const int32_t* __restrict__ blk_inst,
                                                           const double* __restrict__ values, double* __restrict__ gp) {
  const int blk = (int)(blockIdx.x / (unsigned)L.g_blocks);
  const int lb = (int)(blockIdx.x - (unsigned)blk * (unsigned)L.g_blocks);
  int ii[R];
#pragma unroll
  for (int r = 0; r < R; ++r) ii[r] = __builtin_amdgcn_readfirstlane(blk_inst[blk * R + r]);
  const StaffBatchTable tb = tabs[inst[ii[0]].table];
  const int n_rows = tb.n_rows;
  const int e_own = lb * 64 + (int)threadIdx.x;
  const int e = e_own < L.n_levels ? e_own : L.n_levels - 1;  // (lanes past the last level repeat it and store nothing)
  const int y = L.y0 + e;
  const int row = y >= n_rows - 1 ? n_rows - 1 : y;
  const int nj = tb.row_len[row];
  int kmax = nj, kmin = nj;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    kmax = max(kmax, __shfl_xor(kmax, off, 64));
    kmin = min(kmin, __shfl_xor(kmin, off, 64));
  }
  kmax = __builtin_amdgcn_readfirstlane(kmax);
  kmin = __builtin_amdgcn_readfirstlane(kmin);
  const char* pb = reinterpret_cast<const char*>(tb.pT);
  const char* vb[R];
  double salary[R], pen[R], msd[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const StaffBatchInst& I = inst[ii[r]];
    vb[r] = reinterpret_cast<const char*>(values + (FUTURE ? I.v_next_off : 0));
    salary[r] = I.salary;
    pen[r] = I.pen;
    msd[r] = (double)I.min_staff;
  }
  const uint32_t row_bytes = (uint32_t)n_rows * 8u;
  const uint32_t row_off = (uint32_t)row * 8u;
  const int yv = y - L.next_x_lo, v_lo = L.nn_lo - L.next_x_lo, v_hi = L.nn_hi - L.next_x_lo;
  const double yd = (double)y;
  auto fetch = [&](int j0, double (&p)[U], double (&vn)[R][U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u < kmax ? j0 + u : kmax - 1;  // (scalar)
      p[u] = *reinterpret_cast<const double*>(pb + ((uint32_t)j * row_bytes + row_off));
      if constexpr (FUTURE) {
        int i = yv - j;
        i = i > v_hi ? v_hi : i;
        i = i < v_lo ? v_lo : i;
#pragma unroll
        for (int r = 0; r < R; ++r) vn[r][u] = *reinterpret_cast<const double*>(vb[r] + (uint32_t)(i * 8));
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) vn[r][u] = 0.0;
      }
    }
  };
  double g[R], ps = 0.0;
#pragma unroll
  for (int r = 0; r < R; ++r) g[r] = 0.0;
  auto steps = [&](auto guard_tag, int j0, const double (&p)[U], const double (&vn)[R][U]) {
    constexpr bool GUARD = decltype(guard_tag)::value;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u;
      if (!GUARD || j < nj) {
        const double nd = yd - (double)j;  // (double)nextStaffNum
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const double penalty = nd > msd[r] ? 0.0 : pen[r] * (msd[r] - nd);
          const double w = salary[r] * nd + penalty;
          g[r] += p[u] * w;
          if constexpr (FUTURE) g[r] += p[u] * vn[r][u];
        }
        ps += p[u];
      }
    }
  };
  double pa[U], va[R][U], pb2[U], vb2[R][U];
  fetch(0, pa, va);
  int j0 = 0;
  for (; j0 + 2 * U <= kmin; j0 += 2 * U) {  // inside every row of the wave
    fetch(j0 + U, pb2, vb2);
    steps(std::false_type{}, j0, pa, va);
    fetch(j0 + 2 * U, pa, va);
    steps(std::false_type{}, j0 + U, pb2, vb2);
  }
  for (; j0 < kmax; j0 += 2 * U) {
    fetch(j0 + U, pb2, vb2);
    steps(std::true_type{}, j0, pa, va);
    fetch(j0 + 2 * U, pa, va);
    steps(std::true_type{}, j0 + U, pb2, vb2);
  }
  if (e_own < L.n_levels) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r > 0 && ii[r] == ii[r - 1]) continue;  // a spare slot of a short block
      double* row_g = gp + (int64_t)ii[r] * 2 * L.lev_stride;
      row_g[e_own] = g[r];
      row_g[L.lev_stride + e_own] = ps;
    }
  }
}

// staff_sep_min_kernel (sdp_staff_sep.hpp) for the batch: workgroup = (instance, 64 states) x 4 action strides; the strict
// compare from (Double.MAX_VALUE, 0) per stride in ascending action, the four combined in (value, action) order.
__global__ __launch_bounds__(256) void staff_batch_min_kernel(StaffBatchLaunch L, const StaffBatchInst* __restrict__ inst,
                                                              const double* __restrict__ gp, double* __restrict__ values,
                                                              int32_t* __restrict__ policy) {
  __shared__ double s_val[256];
  __shared__ int s_k[256];
  const int i = (int)(blockIdx.x / (unsigned)L.tiles);
  const int tile = (int)(blockIdx.x - (unsigned)i * (unsigned)L.tiles);
  const StaffBatchInst& I = inst[i];
  const double K = I.K, v = I.v;
  const int tid = threadIdx.x;
  const int sx = tid & 63, as = tid >> 6;
  const int i0 = tile * 64;
  double best = 1.7976931348623157e308;
  int bestk = 0;
  if (i0 + sx < L.n_states) {
    const double* gs = gp + (int64_t)i * 2 * L.lev_stride + i0 + sx;  // level of (state, action k): entry state + k
    const double* pp = gs + L.lev_stride;
#pragma unroll 4
    for (int k = as; k < L.n_actions; k += 4) {
      const double q = ((k > 0 ? K : 0.0) + v * (double)k) * pp[k] + gs[k];
      if (q < best) {
        best = q;
        bestk = k;
      }
    }
  }
  s_val[tid] = best;
  s_k[tid] = bestk;
  __syncthreads();
  const int idx = i0 + tid;
  if (tid < 64 && idx < L.n_states) {
    double bv = s_val[tid];
    int bk = s_k[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const double ov = s_val[w * 64 + tid];
      const int ok = s_k[w * 64 + tid];
      if (better<false>(ov, ok, bv, bk)) {
        bv = ov;
        bk = ok;
      }
    }
    values[I.v_cur_off + idx] = bv;
    policy[I.pol_off + idx] = bk;
  }
}

// V_1(iniStaffNum) and its hire index of every instance
__global__ __launch_bounds__(256) void staff_batch_initial_kernel(const StaffBatchInst* __restrict__ inst, int n, int ini_idx,
                                                                  const double* __restrict__ values,
                                                                  const int32_t* __restrict__ policy,
                                                                  double* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out_val[i] = values[inst[i].v_cur_off + ini_idx];
  out_idx[i] = policy[inst[i].pol_off + ini_idx];
}

}  // namespace sdp
