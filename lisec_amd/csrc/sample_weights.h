// Sample weights of the loss passes (include/lisec_hip.h, lisec_sample_weights): what the WEIGHTED instantiations of
// k_head_loss, k_det_loss and k_det_iou read, and the host check of the descriptor.  A weight is a device float per output:
// one for the sweep, or one per cell of the (Ho, Wo) grid.  It is read when the launch runs, so a replayed plan sees
// whatever was staged at that address.  Output 0 is the class output (channels 0, 1 of a cell), output 1 the regression
// output (channels 2..15).
#pragma once
#include "common.h"

namespace lisec {

struct CellWeights {                 // the descriptor by value: a kernel argument
    const float* w[2];               // nullptr: weight 1
    int per_cell[2];
    unsigned metrics[2];             // head loss: bit j = metric j of output o is weighted
};

inline CellWeights cell_weights(const lisec_sample_weights& sw) {
    return {{sw.w[0], sw.w[1]}, {sw.per_cell[0], sw.per_cell[1]}, {sw.weighted_metrics[0], sw.weighted_metrics[1]}};
}

// n_metrics == nullptr: an entry without weighted metrics (the detection losses)
inline int check_sample_weights(const lisec_sample_weights* sw, const int* n_metrics) {
    LISEC_CHECK_ARG(sw, "sample weights: NULL descriptor");
    LISEC_CHECK_ARG(sw->struct_bytes == (int)sizeof(lisec_sample_weights),
                    "sample weights: descriptor of %d bytes, this library's has %d", sw->struct_bytes,
                    (int)sizeof(lisec_sample_weights));
    for (int o = 0; o < 2; ++o) {
        LISEC_CHECK_ARG(sw->per_cell[o] == 0 || sw->per_cell[o] == 1, "sample weights: per_cell[%d] must be 0 or 1 (got %d)",
                        o, sw->per_cell[o]);
        const int n = n_metrics ? n_metrics[o] : 0;
        LISEC_CHECK_ARG((sw->weighted_metrics[o] >> n) == 0u,
                        "sample weights: output %d has a weighted-metric bit at or above the %d metrics it may weigh", o, n);
    }
    return LISEC_OK;
}

#ifdef __HIPCC__
// A loss kernel is `template <bool WEIGHTED, typename... W>` with `W... cw` as its last parameter: no parameter in the
// unweighted instantiation -- its parameter list and its code stay what they were before there were weights -- and one
// CellWeights in the weighted one, which reads it through the_weights(cw...).
__device__ __forceinline__ CellWeights the_weights() { return {}; }
__device__ __forceinline__ const CellWeights& the_weights(const CellWeights& cw) { return cw; }

// The per-sweep weights of both outputs (1 where an output has a map or no weights): the same address on every lane, so
// the loads are scalar and sit in front of the grid-stride loop.
struct SweepWeights {
    float s[2];
};
__device__ __forceinline__ SweepWeights sweep_weights(const CellWeights& cw) {
    SweepWeights r;
    r.s[0] = cw.w[0] && !cw.per_cell[0] ? cw.w[0][0] : 1.f;
    r.s[1] = cw.w[1] && !cw.per_cell[1] ? cw.w[1][0] : 1.f;
    return r;
}
// The weight of cell m for output o: the lanes of a cell that share an output read one address.
__device__ __forceinline__ float cell_weight(const CellWeights& cw, const SweepWeights& sw, int o, long long m) {
    const float* p = o ? cw.w[1] : cw.w[0];
    const bool map = p && (o ? cw.per_cell[1] : cw.per_cell[0]);
    return map ? p[m] : (o ? sw.s[1] : sw.s[0]);
}
#endif

}  // namespace lisec
