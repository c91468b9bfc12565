// ONE PASS of window_f1_level_kernel (sdp_window.hpp) over the level block y0 from step j_first, with RW action rows.  This
// file is the kernel's text, included inside its level-block loop once per row count -- not a header of its own:
//     SDP_LEVEL_PASS_ROWS   RW: R (an exact pass, or a screened one with RS = R) or the RS screen rows
//     SDP_LEVEL_PASS_C0     c0 (R rows) or c0s (row q stands for rows q G .. (q + 1) G - 1, G = R / RW: THE SCREEN ROWS)
//     SDP_LEVEL_PASS_ACC    the sums: double [RW][S]
// One text for both, as f1_cells is one body for the one-action launches: the same operations on the same operands in the
// same order.  (Two inclusions and not a lambda or a function called twice: wrapped in a closure the very same statements
// take 263 instead of 209 VGPRs, one wave per SIMD -- profiles/f1_screen_rows_resources.txt.)  Only the cut-off's test knows
// about the collapse: it reads the R thresholds of a level and holds each against the sum of the row that stands for it.
// The kernel's SG (THE STEP GROUPS, sdp_window.hpp) orders the instructions of a step, in either pass, and nothing else.
    {
      constexpr int RW = SDP_LEVEL_PASS_ROWS, G = R / RW;
      static_assert(RW >= 1 && R % RW == 0, "screen rows divide R");
      double imm[RW][S];  // ring: at step j, cell s uses imm[r][(s - j) mod S] = c0[r] + M(y0 + s - j)
#pragma unroll
      for (int s = 0; s < S; ++s) {
        const double ms = window_entry<false, false>(W, nullptr, nullptr, y0 + s - j_first).x;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          SDP_LEVEL_PASS_ACC[r][s] = 0.0;
          imm[r][s] = SDP_LEVEL_PASS_C0[r] + ms;
        }
      }
      [[maybe_unused]] int cut_at = max(cut_first, j_first + S);
      cut_fail = 0;
      stop_at = -1;
      // (PF) the step the task's next block is expected to start at: screened if this block stops, as the one before did
      [[maybe_unused]] int pf_next = 0;
      if constexpr (CUT && PF) pf_next = pf_stop != INT32_MAX && (j_first > 0 || scr_run + 1 >= scr_need) ? L.screen_start : 0;
      for (int j0 = j_first; j0 < L.d_pad && stop_at < 0; j0 += DB) {
        const int nj = min(DB, L.d_pad - j0);
        // the table of steps j0 .. j0 + nj - 1: lane t forms row t (rows past nj repeat the last step and are not read)
        __builtin_amdgcn_wave_barrier();
        const bool fetched = PF && pf_y == y0 && pf_j == j0;  // (wave-uniform)
        if constexpr (PF) {
          if (fetched) {
            // the window goes through a strip at the start of the table region (the table before is dead, and the rows are
            // written only after every lane has read its S entries)
            s_row[lane] = level_v_decode<KEYED_IN>(pf_w0);
            if (lane < DB + S - 1 - 64) s_row[64 + lane] = level_v_decode<KEYED_IN>(pf_w1);
            __builtin_amdgcn_wave_barrier();
          }
        }
        if (lane < DB) {
          const int tt = min(lane, nj - 1);
          const int j = j0 + tt;
          double p;
          double* row = s_row + lane * ROW;
          double vv[S];
          if (fetched) {
            p = pf_p;
#pragma unroll
            for (int s = 0; s < S; ++s) vv[s] = s_row[DB - 1 - tt + s];
          } else {
            p = pmf_p[j];  // (the array ends in kPmfPad zeros: d_pad < D + S stays inside)
            if constexpr (FUTURE) {
#pragma unroll
              for (int s = 0; s < S; ++s) vv[s] = level_v<KEYED_IN>(W, v_next, k_next, y0 + s - j);
            }
          }
          __builtin_amdgcn_wave_barrier();
          row[0] = p;
          row[1] = window_entry<false, false>(W, nullptr, nullptr, y0 - j - 1).x;
          if constexpr (FUTURE) {
#pragma unroll
            for (int s = 0; s < S; ++s) row[2 + s] = p * vv[s];
          }
        }
        __builtin_amdgcn_wave_barrier();
        // The inputs of the table expected next, in flight under this table's steps: the block's next table if there is one
        // and (CUT) the block before got that far -- after a block that ran to the end, a full run -- else the first table
        // of the task's next block.  A wrong guess costs that table its direct loads and touches nothing else.
        if constexpr (PF) {
          bool same = j0 + DB < L.d_pad;
          if constexpr (CUT) same = same && j0 + DB < pf_stop;
          if (same || y0 + S < ye) prefetch(same ? y0 : y0 + S, same ? j0 + DB : pf_next);
        }
        // Each step reads the NEXT step's row (a broadcast ds_read_b128 per two doubles) before its own 100 fp64
        // instructions, which then cover the LDS latency; the row past the block's last step lies inside the wave's region
        // and is not used.
        constexpr int NQ = FUTURE ? ROW / 2 : 1;
        double2 nxt[NQ];
#pragma unroll
        for (int u = 0; u < NQ; ++u) nxt[u] = reinterpret_cast<const double2*>(s_row)[u];
#pragma unroll 1
        for (int t0 = 0; t0 < nj; t0 += S) {
          if constexpr (CUT) {
            // (the imm ring is in its canonical rotation here; the slots are the ones the epilogue below updates)
            if (j0 + t0 >= cut_at) {
              const int sb = (y0 - yb) - lane + NA - 1;
              // (`beaten` is a pure conjunction.  With a future term the R thresholds of a level are read together and the
              // compares ANDed without a short cut -- S LDS round trips per test instead of R S; every slot index lies inside
              // the wave's slots.  Period T keeps the short cut: the grouped reads cost it the third wave per SIMD, 198 VGPRs.)
              bool beaten = true;
#pragma unroll
              for (int s = 0; s < S; ++s) {
                if constexpr (FUTURE || RW < R) {
                  double th[R];
#pragma unroll
                  for (int r = 0; r < R; ++r) th[r] = s_val[sb + s - 64 * r];
#pragma unroll
                  for (int r = 0; r < R; ++r) {
                    const bool live = r == 0 ? (kreal[0] && kb + lane != 0) : kreal[r];  // not a padded action, not action 0
                    beaten = beaten & (!live | (SDP_LEVEL_PASS_ACC[r / G][s] > th[r]));
                  }
                } else {
#pragma unroll
                  for (int r = 0; r < R; ++r) {
                    const bool live = r == 0 ? (kreal[0] && kb + lane != 0) : kreal[r];
                    beaten = beaten && (!live || SDP_LEVEL_PASS_ACC[r][s] > s_val[sb + s - 64 * r]);
                  }
                }
              }
              ++cut_tests;
              if (__builtin_amdgcn_ballot_w64(!beaten) == 0) {
                stop_at = j0 + t0;
                break;
              }
              ++cut_fail;
              cut_at = cut_once ? INT32_MAX : j0 + t0 + S;
            }
          }
          const double* rows = s_row + t0 * ROW;
#pragma unroll
          for (int t = 0; t < S; ++t) {
            double2 cur[NQ];
#pragma unroll
            for (int u = 0; u < NQ; ++u) {
              cur[u] = nxt[u];
              nxt[u] = reinterpret_cast<const double2*>(rows + (t + 1) * ROW)[u];
            }
            // (fences: left to itself the scheduler pulls the next step's products up to the reads and waits on them at once)
            __builtin_amdgcn_sched_barrier(0);
            const double2 pm = cur[0];
            const double p = pm.x;
            double pv[S];
            if constexpr (FUTURE) {
#pragma unroll
              for (int s = 0; s < S; s += 2) {
                pv[s] = cur[1 + s / 2].x;
                if (s + 1 < S) pv[s + 1] = cur[1 + s / 2].y;
              }
            }
            if constexpr (SG == 1) {
#pragma unroll
              for (int s = 0; s < S; ++s) {
#pragma unroll
                for (int r = 0; r < RW; ++r) {
                  SDP_LEVEL_PASS_ACC[r][s] += p * imm[r][(s - t + S) % S];
                  if constexpr (FUTURE) SDP_LEVEL_PASS_ACC[r][s] += pv[s];
                }
              }
            } else {
              // THE STEP GROUPS: cell c = s RW + r, SG cells at a time -- products, sums, future terms, each kind fenced off,
              // so that an instruction's operand was issued SG instructions before it (per cell: the text above)
#pragma unroll
              for (int cb = 0; cb < RW * S; cb += SG) {
                double prod[SG];
#pragma unroll
                for (int g = 0; g < SG; ++g) prod[g] = p * imm[(cb + g) % RW][((cb + g) / RW - t + S) % S];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < SG; ++g) SDP_LEVEL_PASS_ACC[(cb + g) % RW][(cb + g) / RW] += prod[g];
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (FUTURE) {
#pragma unroll
                  for (int g = 0; g < SG; ++g) SDP_LEVEL_PASS_ACC[(cb + g) % RW][(cb + g) / RW] += pv[(cb + g) / RW];
                  __builtin_amdgcn_sched_barrier(0);
                }
              }
            }
            // level 0 at step j + 1 takes the slot level S - 1 has just used
#pragma unroll
            for (int r = 0; r < RW; ++r) imm[r][(2 * S - 1 - t) % S] = SDP_LEVEL_PASS_C0[r] + pm.y;
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }
