// samsim_row_plan.h -- which layer rows one walk of a diagnostic kernel loads, and which items (functionals, profile sensors) it
// serves.  Plain C++, shared by the host code that fills the plan and the kernels that read it as part of their argument.
//
// An item needs one or two arrays of the layer block (S_bu after a step needs two, S_abs and m).  A walk loads at most
// ROW_PLAN_ROWS distinct arrays beside thick; the items it serves form a group.  The rows are deduplicated within a group and an
// item joins the first group in which the union of the rows still fits (first-fit), else it begins a new one: at most one group per
// item.  Which walk serves an item does not change the item's value.
#ifndef SAMSIM_ROW_PLAN_H
#define SAMSIM_ROW_PLAN_H

#include <cstdint>

#define ROW_PLAN_ROWS 4

template <int MAXG>
struct RowPlan {
  int32_t ngroups;
  int32_t gn[MAXG];                  // rows of each group
  int8_t grow[MAXG][ROW_PLAN_ROWS];  // their arrays (enum samsim_layer_array)
};

// the walk that serves an item and the positions of its arrays among the walk's rows
struct RowPlace { int32_t group, ia, ib; };

// places an item that needs array a and, where b >= 0, array b.  The plan starts zeroed (RowPlan<MAXG>{}) and takes at most MAXG items:
// neither is checked here.
template <int MAXG>
inline RowPlace row_plan_place(RowPlan<MAXG> &p, int a, int b) {
  auto find = [&](int g, int x) { for (int j = 0; j < p.gn[g]; ++j) if (p.grow[g][j] == x) return j; return -1; };
  int g = 0;
  for (; g < p.ngroups; ++g) {
    const int missing = (find(g, a) < 0) + (b >= 0 && find(g, b) < 0);
    if (p.gn[g] + missing <= ROW_PLAN_ROWS) break;
  }
  if (g == p.ngroups) p.gn[p.ngroups++] = 0;
  auto at = [&](int x) {
    int j = find(g, x);
    if (j < 0) { j = p.gn[g]; p.grow[g][p.gn[g]++] = (int8_t)x; }
    return j;
  };
  const int ia = at(a);
  return RowPlace{g, ia, b >= 0 ? at(b) : 0};
}

#endif
