// The "increasing" flag of the extend-add gathers, host code shared by the analysis phase (symbolic.cpp exports it as
// femo_child_maps_increasing, solver/symbolic.py states it in numpy) and the numeric phase (femo_set_frontal_plan uploads it).
//
// A child's boundary rows land in its parent at up_map.  Where that map is strictly increasing, two boundary rows of the child keep
// their order in the parent: for an entry (r, c) of the parent's lower triangle, r >= c, the child rows (x, y) that land there
// satisfy x >= y, so the entry is S_c[x][y] as it stands -- no min / max of the pair -- and its address splits into a term of the
// column alone and the row.  node_order 1 gives every front such a map; node_order 0 (ascending node id) nearly none.
#pragma once
#include <cstdint>

namespace femo {

// the rule: the rows [npiv, nf) of one front's up_map, strictly increasing (an empty or one-row boundary is)
inline bool up_map_increasing(const int32_t* up_bnd, int64_t nb) {
    for (int64_t k = 1; k < nb; ++k)
        if (up_bnd[k] <= up_bnd[k - 1]) return false;
    return true;
}

// per front: bit 0 = the left child's map is increasing, bit 1 = the right child's; a child that is not there counts as increasing
// (nothing of it is gathered).  A front that is neither child of its parent is skipped (femo_set_frontal_plan rejects such a plan).
inline void child_maps_increasing(int32_t ntree, const int32_t* npiv, const int32_t* nf, const int64_t* dof_off, const int32_t* parent,
                                  const int32_t* left, const int32_t* right, const int32_t* up_map, int32_t* flags) {
    for (int32_t t = 0; t < ntree; ++t) flags[t] = 3;
    for (int32_t t = 0; t < ntree; ++t) {
        const int32_t p = parent[t];
        if (p < 0 || p >= ntree) continue;
        if (up_map_increasing(up_map + dof_off[t] + npiv[t], (int64_t)nf[t] - npiv[t])) continue;
        if (left[p] == t) flags[p] &= ~1;
        else if (right[p] == t) flags[p] &= ~2;
    }
}

}   // namespace femo
