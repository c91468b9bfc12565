// sdp_multi_device.hpp -- what the two translation units of the two-product families share: the reachable-set engine
// (sdpgpu_sparse.hip) and the rollout of its policy (sdpgpu_multisim.hip, kernels in sdp_multi_sim.hpp).  The parameter block,
// the state tuple, the model lambdas of the three families (MultiProductLeadtime, MultiItemCash, MultiItemCashXR), the
// successor of a (state, action, demand pair) and the tuple hash exist ONCE: a rollout steps through the statements the solve
// evaluated.  Below them, the host side the two units share: the problem a descriptor describes, the per-thread error text of
// sdpgpu_multilead_last_error and the exception barrier of the entry points.  Internal, header only.
#pragma once
#include "../../include/sdpgpu.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

namespace sdp_multi {

struct MLParams {
  double price[2], vari[2], sal[2];
  double r0, r1, r2, limit, interest_free;
  double min_inventory, max_inventory, min_cash, max_cash, discount;
  double overhead;  // of the period being processed
  int32_t qb;       // actions (i, j), i, j in [0, qb)
  int32_t nd;       // demand pairs, index = i1 * n2 + i2 (GetPmfMulti.java:157-172)
  int32_t is_last;  // period == T: salvage applies, no transition
  int32_t cash_int_cast;  // MultiProductLeadtime.java:219
  int32_t model;          // 0: CashRecursionMultiLead + MultiProductLeadtime lambdas; 1: CashRecursionMulti + MultiItemCash;
                          // 2: CashRecursionMultiXR + MultiItemCashXR (state (x1, x2, R), actions = order-up-to levels)
  double one_minus_deposit;  // model 2: 1 - depositeRate
};

struct Tuple {
  double i1, i2, q1, q2, cash;
};

__device__ __forceinline__ double jmax(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double jmin(double a, double b) { return fmin(a, b); }

// Piecewise overdraft interest, MultiProductLeadtime.java:186-194.
__device__ __forceinline__ double ml_interest(const MLParams& P, double before) {
  double interest;
  if (before >= 0)
    interest = -P.r0 * before;
  else if (before >= -P.interest_free)
    interest = 0;
  else if (before >= -P.limit)
    interest = P.r1 * (-before - P.interest_free);
  else
    interest = P.r2 * (-before - P.limit) + P.r1 * (P.limit - P.interest_free);
  return interest;
}

// Demand-dependent pieces of one state, shared by all actions (MultiProductLeadtime.java:170-183).
struct DemandTerms {
  double revenue, sal_value, next_i1, next_i2;
};

__device__ __forceinline__ DemandTerms demand_terms(const MLParams& P, const Tuple& s, double d1, double d2) {
  DemandTerms t;
  const double end1 = jmax(0.0, s.i1 + s.q1 - d1);
  const double end2 = jmax(0.0, s.i2 + s.q2 - d2);
  const double revenue1 = P.price[0] * jmin(d1, s.i1 + s.q1);
  const double revenue2 = P.price[1] * jmin(s.i2 + s.q2, d2);
  t.revenue = revenue1 + revenue2;
  t.sal_value = P.is_last ? (P.sal[0] * end1 + P.sal[1] * end2) : 0.0;
  // the transition's own end inventories (:210-221): upper clamp on product 1 only, lower clamp on
  // product 2 only, then (int) casts
  double n1 = s.i1 + s.q1 - d1;
  n1 = jmax(0.0, n1);
  double n2 = s.i2 + s.q2 - d2;
  n2 = jmax(0.0, n2);
  n1 = n1 > P.max_inventory ? P.max_inventory : n1;
  n2 = n2 < P.min_inventory ? P.min_inventory : n2;
  t.next_i1 = (double)(int)n1;
  t.next_i2 = (double)(int)n2;
  return t;
}

// cashIncrement of (state, action, demand): MultiProductLeadtime.java:177-198 with the action-only part
// (`bi` = cashBalanceBefore - interest) hoisted by the caller.
__device__ __forceinline__ double cash_increment(const Tuple& s, double bi, const DemandTerms& t) {
  const double after = bi + t.revenue + t.sal_value;
  return after - s.cash;
}

__device__ __forceinline__ double next_cash(const MLParams& P, const Tuple& s, double inc) {
  double c = s.cash + inc;
  c = c > P.max_cash ? P.max_cash : c;
  c = c < P.min_cash ? P.min_cash : c;
  if (P.cash_int_cast) c = (double)(int)c;  // `nextCash = (int) nextCash` (:219)
  return c;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long h, double v) {
  v += 0.0;  // -0.0 -> +0.0 (the reference's equals() compares with ==)
  unsigned long long u = (unsigned long long)__double_as_longlong(v);
  h ^= u + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  return h;
}

__device__ __forceinline__ unsigned long long tuple_hash(const Tuple& t) {
  unsigned long long h = 0x243f6a8885a308d3ull;
  h = mix64(h, t.i1);
  h = mix64(h, t.i2);
  h = mix64(h, t.q1);
  h = mix64(h, t.q2);
  h = mix64(h, t.cash);
  return h;
}

__device__ __forceinline__ bool tuple_eq(const Tuple& a, const Tuple& b) {
  return a.i1 == b.i1 && a.i2 == b.i2 && a.q1 == b.q1 && a.q2 == b.q2 && a.cash == b.cash;
}

// ---- model 1: sdp.cash.multiItem.CashRecursionMulti over the lambdas of cash.multiItem.MultiItemCash ----------
// buildActionList (MultiItemCash.java:66-76): (i, j) is offered iff variCost[0] * i + variCost[1] * j < iniCash + 0.1
__device__ __forceinline__ bool mc_feasible(const MLParams& P, const Tuple& s, int a1, int a2) {
  return P.vari[0] * a1 + P.vari[1] * a2 < s.cash + 0.1;
}

// immediateValue (MultiItemCash.java:79-99)
__device__ __forceinline__ double mc_immediate(const MLParams& P, const Tuple& s, int a1, int a2, double demand1,
                                               double demand2) {
  const double action1 = (double)a1, action2 = (double)a2;
  const double endInventory1 = jmax(0.0, s.i1 + action1 - demand1);
  const double endInventory2 = jmax(0.0, s.i2 + action2 - demand2);
  const double revenue1 = P.price[0] * (s.i1 + action1 - endInventory1);
  const double revenue2 = P.price[1] * (s.i2 + action2 - endInventory2);
  const double revenue = revenue1 + revenue2;
  const double orderingCost1 = P.vari[0] * action1;
  const double orderingCost2 = P.vari[1] * action2;
  const double orderingCosts = orderingCost1 + orderingCost2;
  double salValue = 0;
  if (P.is_last) salValue = P.sal[0] * endInventory1 + P.sal[1] * endInventory2;
  return revenue - orderingCosts + salValue;
}

// stateTransition (MultiItemCash.java:103-118): upper clamp on product 1 only, lower clamp on product 2 only, (int) casts
__device__ __forceinline__ Tuple mc_successor(const MLParams& P, const Tuple& s, int a1, int a2, double demand1,
                                              double demand2) {
  double endInventory1 = s.i1 + (double)a1 - demand1;
  endInventory1 = jmax(0.0, endInventory1);
  double endInventory2 = s.i2 + (double)a2 - demand2;
  endInventory2 = jmax(0.0, endInventory2);
  double nextCash = s.cash + mc_immediate(P, s, a1, a2, demand1, demand2);
  nextCash = nextCash > P.max_cash ? P.max_cash : nextCash;
  nextCash = nextCash < P.min_cash ? P.min_cash : nextCash;
  endInventory1 = endInventory1 > P.max_inventory ? P.max_inventory : endInventory1;
  endInventory2 = endInventory2 < P.min_inventory ? P.min_inventory : endInventory2;
  Tuple n;
  n.cash = (double)(int)nextCash;
  n.i1 = (double)(int)endInventory1;
  n.i2 = (double)(int)endInventory2;
  n.q1 = 0.0;
  n.q2 = 0.0;
  return n;
}

// ---- model 2: sdp.cash.multiItem.CashRecursionMultiXR over the lambdas of cash.multiItem.MultiItemCashXR ------
// The state is (x1, x2, R) with R = cash + variCost . x (kept in Tuple::cash); an action is a pair of order-up-to
// levels (y1, y2) = ((int) x1 + i, (int) x2 + j), i, j in [0, Qbound) (MultiItemCashXR.java:92-105).
// immediateValue (MultiItemCashXR.java:108-128)
__device__ __forceinline__ double xr_immediate(const MLParams& P, const Tuple& s, double action1, double action2,
                                               double demand1, double demand2) {
  const double endInventory1 = jmax(0.0, action1 - demand1);
  const double endInventory2 = jmax(0.0, action2 - demand2);
  const double revenue1 = P.price[0] * (action1 - endInventory1);
  const double revenue2 = P.price[1] * (action2 - endInventory2);
  const double revenue = revenue1 + revenue2;
  const double initialCash = s.cash - P.vari[0] * s.i1 - P.vari[1] * s.i2;
  const double orderingCostY1 = P.vari[0] * action1;
  const double orderingCostY2 = P.vari[1] * action2;
  const double orderingCostsY = orderingCostY1 + orderingCostY2;
  double salValue = 0;
  if (P.is_last) salValue = P.sal[0] * endInventory1 + P.sal[1] * endInventory2;
  return revenue + P.one_minus_deposit * (s.cash - orderingCostsY) + salValue - initialCash;
}

// stateTransition (MultiItemCashXR.java:132-148)
__device__ __forceinline__ Tuple xr_successor(const MLParams& P, const Tuple& s, double action1, double action2,
                                              double demand1, double demand2) {
  double endInventory1 = action1 - demand1;
  endInventory1 = jmax(0.0, endInventory1);
  double endInventory2 = action2 - demand2;
  endInventory2 = jmax(0.0, endInventory2);
  const double initialCash = s.cash - P.vari[0] * s.i1 - P.vari[1] * s.i2;
  double nextCash = initialCash + xr_immediate(P, s, action1, action2, demand1, demand2);
  nextCash = nextCash > P.max_cash ? P.max_cash : nextCash;
  nextCash = nextCash < P.min_cash ? P.min_cash : nextCash;
  endInventory1 = endInventory1 > P.max_inventory ? P.max_inventory : endInventory1;
  endInventory2 = endInventory2 < P.min_inventory ? P.min_inventory : endInventory2;
  nextCash = (double)(int)nextCash;
  endInventory1 = (double)(int)endInventory1;
  endInventory2 = (double)(int)endInventory2;
  Tuple n;
  n.i1 = endInventory1;
  n.i2 = endInventory2;
  n.q1 = 0.0;
  n.q2 = 0.0;
  n.cash = (double)(int)nextCash + P.vari[0] * endInventory1 + P.vari[1] * endInventory2;  // nextR
  return n;
}

// The successor of (state, action a, demand j).
__device__ __forceinline__ Tuple successor(const MLParams& P, const Tuple& s, int a, const double2* dem, int j) {
  const int a1 = a / P.qb, a2 = a - a1 * P.qb;
  if (P.model == 1) {
    // an action the state is not offered has no successors of its own: it stands in for (0, 0), which is always
    // offered (0 < cash + 0.1 with cash >= min_cash >= 0), so the candidate list gains nothing new
    const bool ok = mc_feasible(P, s, a1, a2);
    return mc_successor(P, s, ok ? a1 : 0, ok ? a2 : 0, dem[j].x, dem[j].y);
  }
  if (P.model == 2)
    return xr_successor(P, s, (double)((int)s.i1 + a1), (double)((int)s.i2 + a2), dem[j].x, dem[j].y);
  const double oc = P.vari[0] * (double)a1 + P.vari[1] * (double)a2;
  const double before = s.cash - oc - P.overhead;
  const double bi = before - ml_interest(P, before);
  const DemandTerms t = demand_terms(P, s, dem[j].x, dem[j].y);
  Tuple n;
  n.i1 = t.next_i1;
  n.i2 = t.next_i2;
  n.q1 = (double)a1;
  n.q2 = (double)a2;
  n.cash = next_cash(P, s, cash_increment(s, bi, t));
  return n;
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// What a descriptor describes, as the engine reads it: the per-period joint tiles (pairs as the recursion casts them,
// probabilities in list order), the parameter block without its per-period fields, the period-1 state.
struct Problem {
  int T = 0;
  MLParams P{};
  double overhead[16] = {0};
  Tuple ini{};
  std::vector<int> off;  // demand pairs of period t+1: [off[t], off[t+1])
  std::vector<double2> dem;
  std::vector<double> prob;
};

// sdpgpu_sparse.hip: the descriptor checks of sdpgpu_multilead_solve / sdpgpu_multicash_solve / sdpgpu_multixr_solve and the
// problem they hand to the engine (model 1: MultiItemCash, 2: MultiItemCashXR); a refusal leaves its text in ml_error()
int multilead_problem(const sdpgpu_multilead* k, Problem* out);
int multicash_problem(const sdpgpu_multicash* k, int model, double deposit_rate, Problem* out);

std::string& ml_error();    // sdpgpu_sparse.hip: the calling thread's text behind sdpgpu_multilead_last_error()
void ml_test_throw_hook();  // sdpgpu_sparse.hip: SDPGPU_TEST_THROW (tests of the barrier, no device needed)
sdpgpu_multi_table* ml_table();  // sdpgpu_sparse.hip: the calling thread's sdpgpu_multi_set_table request (sdpgpu_multiv.hip fills it too)

// No C++ exception crosses the C ABI: ml_guard wraps the body of every two-product entry point.
template <class Body>
int ml_guard(const char* who, Body&& body) {
  try {
    ml_test_throw_hook();
    return body();
  } catch (const std::bad_alloc&) {
    ml_error() = std::string(who) + ": host allocation failed (std::bad_alloc)";
    return SDPGPU_ERR_ALLOC;
  } catch (const std::exception& e) {
    ml_error() = std::string(who) + ": internal error: " + e.what();
    return SDPGPU_ERR_INTERNAL;
  } catch (...) {
    ml_error() = std::string(who) + ": internal error (unknown exception)";
    return SDPGPU_ERR_INTERNAL;
  }
}

}  // namespace sdp_multi
